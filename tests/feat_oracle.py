"""The oracle's first-hit features (oracle.features: the feature kernel's fp32
mirror and its same-draw fp64 partner) for the scenes the feature tests share
-- tests/test_oracle_features.py (CPU), tests/test_gpu_feat_oracle.py,
tests/test_denoise_host.py and tests/test_gpu_denoise.py -- and NumPy
restatements of fix24 and of rt_feat_resolve.  Results are computed once per
process and read-only.

rtclj is imported inside the functions: the GPU tests load torch first
(tests/conftest.py gpu_lib).
"""
import functools

import numpy as np

import edge_scenes as E
import oracle

ONE = 1 << 24


def scene_args(sc, cam):
    return (sc.sphere.astype(np.float64), sc.kind, sc.mat.astype(np.float64), cam.as_list(), cam.defocus)


def _freeze(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def mirror(sc, cam, w, h, spp, seed, begin=0, rejection=False, **kw):
    """The feature kernel's fp32 mirror: what rt_feat_read returns after one pass."""
    mode = oracle.MODE_MIRROR32 | (0 if rejection else oracle.DIRECT)
    return _freeze(oracle.features(mode, *scene_args(sc, cam), w, h, spp, seed=seed, sample_begin=begin,
                                   nthreads=E.NT, **kw))


def ref64(sc, cam, w, h, spp, seed, begin=0, rejection=False, **kw):
    """The same draws in double (MODE_REF64D; with the rejection disk MODE_REF64)."""
    mode = oracle.MODE_REF64 if rejection else oracle.MODE_REF64D
    return _freeze(oracle.features(mode, *scene_args(sc, cam), w, h, spp, seed=seed, sample_begin=begin,
                                   nthreads=E.NT, **kw))


def add(a, b):
    """Two passes' (sums, hits, depth) into one, as rt_launch_feat's atomics do."""
    return dict(sums=a["sums"] + b["sums"], hits=a["hits"] + b["hits"], depth=np.minimum(a["depth"], b["depth"]))


@functools.lru_cache(maxsize=None)
def edge_mirror(name, spp=E.SPP, begin_offset=0, rejection=False, detail=False):
    """An edge case's mirror features, 64 x 36: `spp` samples from the case's
    sample_begin + begin_offset, the case's seed.  detail: with body, t, rays."""
    sc, cam, meta = E.case(name)
    p = E.params(meta)
    kw = dict(want_body=True, want_t=True, want_rays=True) if detail else {}
    return mirror(sc, cam, E.W, E.H, spp, p["seed"], p["sample_begin"] + begin_offset, rejection, **kw)


@functools.lru_cache(maxsize=None)
def edge_ref64(name, rejection=False):
    sc, cam, meta = E.case(name)
    p = E.params(meta)
    return ref64(sc, cam, E.W, E.H, E.SPP, p["seed"], p["sample_begin"], rejection, want_body=True, want_t=True)


# the denoiser's edge pipelines (tests/test_denoise_host.py, tests/test_gpu_denoise.py): albedo floor
# on every pixel, colours up to 256, depths near 2^-60 and 2^66, a frame that is all sky
DENOISE_CASES = ("albedo_gt1", "albedo_negative", "albedo_saturating", "nonfinite_65", "camera_inside_glass",
                 "ties_big", "scale_2^-62", "scale_2^20", "scale_2^62", "scale_2^63")


@functools.lru_cache(maxsize=None)
def denoise_inputs(name):
    """(half0, half1, feat) of an edge case from the oracle alone: the path
    mirror's frames of 8 spp at sample_begin 0 and 8 (64 x 36, depth 12, the
    case's seed) and the feature mirror's 16 spp, resolved."""
    half0 = E.mirror(name, spp=8, sample_begin=0)[0]
    half1 = E.mirror(name, spp=8, sample_begin=8)[0]
    m = edge_mirror(name)
    feat = resolve_np(m["sums"], m["hits"], m["depth"], E.SPP)
    feat.setflags(write=False)
    return half0, half1, feat


def fix24(c):
    """The kernel's fix24 of float32 colours: c * 2^24 toward zero as uint32,
    NaN and c <= 0 give 0, 2^32 and above 2^32 - 1 -> uint64 array."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(c, np.float32) * np.float32(ONE)
        pos = v > 0
        big = v >= np.float32(2.0 ** 32)
        return np.where(big, np.uint64(0xffffffff), np.where(pos & ~big, v, 0).astype(np.uint64))


def body_albedo_fix24(sc):
    """Per body, what a hit adds to the albedo sums (::attenuation by kind): (n + 1, 3)
    uint64, row -1 (a miss) zero."""
    out = np.zeros((len(sc.kind) + 1, 3), np.uint64)
    opaque = (sc.kind == E.LAMB) | (sc.kind == E.METAL)
    out[:-1][opaque] = fix24(sc.mat[opaque, :3])
    out[:-1][sc.kind == E.GLASS] = ONE
    return out


def resolve_np(sums, hits, depth, samples):
    """rt_feat_resolve restated: float32(sum) * 2^-24 / nf, each step one fp32 operation."""
    nf = np.float32(max(samples, 1))
    out = np.full(hits.shape + (8,), np.nan, np.float32)
    out[..., 0:3] = sums[..., 0:3].astype(np.uint64).astype(np.float32) * np.float32(2.0 ** -24) / nf
    out[..., 3:6] = sums[..., 3:6].astype(np.float32) * np.float32(2.0 ** -24) / nf
    out[..., 6] = depth
    out[..., 7] = hits.astype(np.float32) / nf
    return out
