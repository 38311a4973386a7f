"""Shared by tests/test_gpu_list_modes.py: the three variants a case runs under,
the comparison (tests/test_gpu_body_list.py's), the oracle's fp32 mirror with a
cache, and one launch into pre-filled buffers.

rtclj and torch are imported inside the functions: the GPU tests load torch
first (tests/conftest.py gpu_lib).
"""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np

import oracle
from test_gpu_body_list import _same, _variant

WALK, LIST, DEFAULT = 30, 22, 0
DEPTH = 6
NT = min(16, os.cpu_count() or 1)


def each_variant(run, variants=(WALK, LIST, DEFAULT)):
    """{v: run(v)} with the selector set to v around each call."""
    from rtclj._lib import lib
    got = {}
    old = _variant(variants[0])
    try:
        for v in variants:
            _variant(v)
            got[v] = run(v)
    finally:
        lib.rt_set_variant(old)
    return got


def resolved(ds, p, v):
    """The launch (ds, p) runs the variant the case means: the list's kernel for
    22 and for the default choice, the walk's for 30 (rt_launch_occupancy)."""
    from rtclj._lib import check, lib
    out4 = (C.c_int * 4)()
    check(lib.rt_launch_occupancy(ds, C.byref(p), out4))
    assert out4[3] == (WALK if v == WALK else LIST), (v, list(out4))


@contextmanager
def uploaded(sc, library=None):
    """A fresh upload of sc on device 0: its streams have no tile-cost record."""
    import torch
    from rtclj._lib import check, lib
    dll = library if library is not None else lib
    ds = C.c_void_p()
    check(dll.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    try:
        yield ds
    finally:
        torch.cuda.synchronize()
        dll.rt_scene_free(ds)


def launch(ds, cam, p, stream=None):
    """One rt_launch into a NaN-filled buffer, waited for: (frame, (segments, samples))."""
    import torch
    from rtclj._lib import check, lib
    rows = check(lib.rt_rows_out(C.byref(p)))
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        out = torch.full((rows * p.width * 3,), float("nan"), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    s.synchronize()
    check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()),
                        C.c_void_p(s.cuda_stream)))
    s.synchronize()
    frame = out.cpu().numpy().reshape(rows, p.width, 3)
    assert not np.isnan(frame).any(), "a pixel was not written"
    return frame, tuple(cnt.cpu().tolist())


def same(got, want, what=""):
    """Frame bits and both counters."""
    _same(want, got, what)


def _mode(flags):
    from rtclj._lib import RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS
    assert flags in (0, RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS)
    if flags == RT_FLAG_REALM:
        return oracle.MODE_REALM32 | oracle.DIRECT
    return oracle.MODE_MIRROR32 | (0 if flags == RT_FLAG_REJECTION_SAMPLERS else oracle.DIRECT)


_MIRRORS = {}


def mirror(key, sc, cam, w, h, spp, seed, flags=0, begin=0, bands=None):
    """The oracle's fp32 mirror of the frame: (frame, (segments, samples)), read-
    only and cached per (key, spp, seed, flags, begin, bands).  key names the
    scene and camera; bands: the row ranges of an interleaved shard, in order."""
    k = (key, w, h, spp, seed, flags, begin, bands)
    if k not in _MIRRORS:
        parts = [oracle.render(_mode(flags), sc.sphere.astype(np.float64), sc.kind, sc.mat.astype(np.float64),
                               cam.as_list(), cam.defocus, w, h, spp, DEPTH, seed=seed, sample_begin=begin, rows=rows,
                               nthreads=NT) for rows in (bands or (None,))]
        frame = np.concatenate([f for f, _, _, _ in parts])
        frame.setflags(write=False)
        _MIRRORS[k] = (frame, (sum(s for _, _, s, _ in parts), sum(n for _, _, _, n in parts)))
    return _MIRRORS[k]


def mirror_ints(key, sc, cam, w, h, index, seed, flags=0):
    """Sample `index` alone as the integer sums a pass adds: a 1-spp mirror frame
    is RN(float(sum)) * 2^-24 with sum <= 2^24, exactly an integer.  uint64 (h, w, 3)."""
    f = mirror(key, sc, cam, w, h, 1, seed, flags, begin=index)[0].astype(np.float64) * 2.0 ** 24
    assert np.array_equal(f, np.floor(f)) and f.min() >= 0 and f.max() <= 2 ** 24
    return f.astype(np.uint64)


def shard_bands(h, tile, first, step):
    return tuple((t, min(t + tile, h)) for t in range(tile * first, h, tile * step))


def per_pixel(tiles, rows, width):
    """A (gy, gx) array spread over its tiles' pixels."""
    return np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)[:rows, :width]
