"""The first-hit features' host side (no GPU needed): rt_feat_resolve_host
against a NumPy restatement of include/rt.h's definition, its argument errors,
and the new entries' presence and signatures."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FEAT_FUNCS = ("rt_feat_create", "rt_feat_free", "rt_feat_clear", "rt_feat_samples", "rt_launch_feat",
              "rt_feat_resolve", "rt_feat_read", "rt_feat_resolve_host")


def resolve_numpy(sums, hits, depth, samples):
    """rt.h: albedo / normal = RN(float(sum)) * 2^-24 / RN(float(n)), the albedo
    sums read as unsigned; depth as it is; coverage = RN(float(hits)) / RN(float(n));
    n = max(samples, 1).  Every step one fp32 operation."""
    nf = np.float32(max(int(samples), 1))
    out = np.empty(hits.shape + (8,), np.float32)
    out[..., 0:3] = sums[..., 0:3].view(np.uint64).astype(np.float32) * np.float32(2.0 ** -24) / nf
    out[..., 3:6] = sums[..., 3:6].astype(np.float32) * np.float32(2.0 ** -24) / nf
    out[..., 6] = depth
    out[..., 7] = hits.astype(np.float32) / nf
    return out


def resolve_host(sums, hits, depth, samples):
    from rtclj._lib import fptr, i64ptr, lib, u32ptr
    out = np.full(hits.shape + (8,), np.nan, np.float32)
    rc = lib.rt_feat_resolve_host(i64ptr(sums), u32ptr(hits), fptr(depth), hits.size, samples, fptr(out))
    assert rc == 0, lib.rt_last_error()
    return out


@pytest.mark.parametrize("samples", [0, 1, 7, (1 << 24) + 1, (1 << 32) - 1])
def test_resolve_host_equals_the_definition(samples):
    rng = np.random.default_rng(5 + samples % 97)
    n = 4096
    s = max(samples, 1)
    sums = np.empty((n, 6), np.int64)
    # albedo: up to samples x (a colour's clamp, 2^32 - 1); normals: both signs, |n| <= 1 per sample
    sums[:, 0:3] = (rng.integers(0, 1 << 32, (n, 3), dtype=np.int64) * rng.integers(0, s + 1, (n, 3), dtype=np.int64))
    sums[:, 3:6] = rng.integers(-(s << 24), (s << 24) + 1, (n, 3), dtype=np.int64)
    hits = rng.integers(0, s + 1, n, dtype=np.int64).astype(np.uint32)
    depth = rng.uniform(1e-3, 1e3, n).astype(np.float32)
    # the edges: nothing hit (0, +inf), every sample hit, the largest and smallest sums
    hits[0], depth[0], sums[0] = 0, np.inf, 0
    hits[1] = s
    sums[2, 3:6] = (-(s << 24), s << 24, -1)
    sums[3, 0:3] = (0, 1, s << 24)
    want = resolve_numpy(sums, hits, depth, samples)
    got = resolve_host(sums, hits, depth, samples)
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0, 6] == np.inf and got[0, 7] == 0 and not got[0, :6].any()
    assert got[1, 7] == np.float32(s) / np.float32(s) == 1.0
    assert got[2, 3] == -1.0 and got[2, 4] == 1.0 and got[2, 5] < 0
    if samples <= 1:
        assert got[3, 2] == 1.0


def test_albedo_sums_are_read_as_unsigned():
    """A channel's clamp is 2^32 - 1 per sample: 2^32 - 1 samples of it pass 2^63."""
    sums = np.zeros((1, 6), np.int64)
    big = np.uint64((1 << 32) - 1) * np.uint64((1 << 32) - 1)
    sums.view(np.uint64)[0, 0] = big
    got = resolve_host(sums, np.zeros(1, np.uint32), np.full(1, np.inf, np.float32), (1 << 32) - 1)
    assert got[0, 0] == np.float32(big) * np.float32(2.0 ** -24) / np.float32(2.0 ** 32) > 0


def test_argument_errors():
    from rtclj._lib import fptr, i64ptr, lib, u32ptr
    sums, hits = np.zeros((2, 6), np.int64), np.zeros(2, np.uint32)
    depth, out = np.zeros(2, np.float32), np.zeros((2, 8), np.float32)
    ok = (i64ptr(sums), u32ptr(hits), fptr(depth), 2, 1, fptr(out))
    assert lib.rt_feat_resolve_host(*ok) == 0
    for k in (0, 1, 2, 5):
        bad = list(ok)
        bad[k] = None
        assert lib.rt_feat_resolve_host(*bad) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_feat_resolve_host(None, None, None, 0, 1, None) == 0      # nothing to do
    for samples in (-1, 1 << 32):
        assert lib.rt_feat_resolve_host(*ok[:4], samples, ok[5]) == -1 and b"samples" in lib.rt_last_error()
    # the device entries refuse NULL handles before any device call
    assert lib.rt_feat_create(None, None, None) == -1
    assert lib.rt_launch_feat(None, None, None, None, None, None) == -1
    assert lib.rt_feat_resolve(None, None, None) == -1
    assert lib.rt_feat_read(None, None, None, None, None) == -1
    assert lib.rt_feat_clear(None, None) == -1
    assert lib.rt_feat_samples(None) == 0 and lib.rt_feat_free(None) == 0


@pytest.mark.parametrize("which", ["product", "diag"])
def test_symbols_and_signatures(which):
    import rtclj
    from rtclj import _lib
    dll = C.CDLL(str(rtclj.library_path if which == "product" else _lib.diag_library_path))
    hdr = (ROOT / "include" / "rt.h").read_text()
    for name in FEAT_FUNCS:
        assert hasattr(dll, name), name
        assert name in _lib.SIGNATURES and name in _lib.ADDITIVE
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    m = re.search(r"#define RT_FEAT_CHANNELS (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.RT_FEAT_CHANNELS == 8
    assert re.search(r"#define RT_ABI_VERSION 3\b", hdr)
    res, args = _lib.SIGNATURES["rt_launch_feat"]
    assert res is C.c_int and len(args) == 6
    assert _lib.SIGNATURES["rt_feat_samples"][0] is C.c_int64
    assert len(_lib.SIGNATURES["rt_feat_read"][1]) == 5 and len(_lib.SIGNATURES["rt_feat_resolve_host"][1]) == 6


def test_python_host_exposes_features():
    from rtclj import raytracing as R
    for name in ("add", "samples", "frame", "raw", "clear", "close", "__enter__", "__exit__"):
        assert hasattr(R.Features, name), name
