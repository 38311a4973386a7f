"""The camera prelude's list of bodies: variant 22 lists
a tile's kept bodies, not their leaf records, and its trip runs list passes of
up to four listed bodies with the exact step per body.  Variant 30 is 22
without the list, every segment through the walk; paths, draws and the
per-body operations are the walk's, so each case renders both and compares the
frame and both counters (segments, samples) bit for bit.

The scenes (tests/body_list_scenes.py) are frames of a few tiles in which some
tile lists exactly n bodies for every n in 0 .. 14 and some tile 15 or more
(no list: the walk), by rt_tile_bodies_host's count; among them two coincident
bodies (a tie the lower index wins; the list pass's repeated slot), lists out
of one leaf record, out of two at differing slots, and out of five and more.
44 x 27 has partial border tiles.  test_the_scenes_hold_every_list_length
asserts all of that before anything is rendered.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle

sys.path.insert(0, str(Path(__file__).resolve().parent))

import body_list_scenes as B  # noqa: E402

pytestmark = pytest.mark.gpu

WALK, LIST = 30, 22
DEPTH = 6


def _variant(v):
    from rtclj._lib import lib
    old = lib.rt_set_variant(v)
    assert old >= 0, f"rt_set_variant({v}) refused"
    return old


def _both(render):
    """render() under the walk and under the list: (frame, counters) each."""
    from rtclj._lib import lib
    got = {}
    old = _variant(WALK)
    try:
        for v in (WALK, LIST):
            _variant(v)
            got[v] = render()
    finally:
        lib.rt_set_variant(old)
    return got[WALK], got[LIST]


def _render(sc, cam, w, h, spp, flags=0, seed=3):
    from rtclj import raytracing as R

    def go():
        st = {}
        out = R.render(sc, cam, w, h, spp=spp, max_depth=DEPTH, seed=seed, n_devices=1, stats=st, flags=flags)
        return out, (st.get("segments"), st.get("samples"))
    return go


def _same(a, b, what=""):
    (fa, ca), (fb, cb) = a, b
    assert fa.shape == fb.shape and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), \
        f"{what}: {float((fa == fb).all(axis=-1).mean()):.4%} pixels bit-exact"
    assert ca == cb, (what, ca, cb)


@pytest.fixture(scope="module")
def frames(gpu_lib):
    return {name: B.frame(name) for name in B.FRAMES}


def test_the_scenes_hold_every_list_length(frames):
    got = [B.describe(B.tile_lists(sc, cam, B.params(w, h))) for sc, cam, w, h in frames.values()]
    print(got)
    missing = set(range(15)) - set().union(*(g["counts"] for g in got))
    assert not missing, f"no tile lists exactly {sorted(missing)} bodies"
    for key in ("overflow", "one_record", "two_records", "five_records"):
        assert any(g[key] for g in got), key


def test_the_launch_runs_the_list_variant(frames):
    from rtclj._lib import check, lib
    sc, cam, w, h = frames["40x24"]
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    old = _variant(LIST)
    try:
        out4 = (C.c_int * 4)()
        p = B.params(w, h, spp=7)
        check(lib.rt_launch_occupancy(ds, C.byref(p), out4))
        assert out4[3] == LIST and out4[0] == 7 and out4[1] <= 72, list(out4)
    finally:
        lib.rt_set_variant(old)
        lib.rt_scene_free(ds)


@pytest.mark.parametrize("sampler", ["direct", "rejection"])
@pytest.mark.parametrize("spp", [1, 7])
@pytest.mark.parametrize("name", sorted(B.FRAMES))
def test_frames(frames, name, spp, sampler):
    from rtclj import _lib
    sc, cam, w, h = frames[name]
    flags = 0 if sampler == "direct" else _lib.RT_FLAG_REJECTION_SAMPLERS
    _same(*_both(_render(sc, cam, w, h, spp, flags)), f"{name} {spp} spp {sampler}")


@pytest.mark.parametrize("name", sorted(B.FRAMES))
def test_realm(frames, name):
    from rtclj import _lib
    sc, cam, w, h = frames[name]
    _same(*_both(_render(sc, cam, w, h, 7, _lib.RT_FLAG_REALM)), f"{name} RT_FLAG_REALM")


def test_defocus(frames):
    """The same bodies under a lens: wider lists, the disk sampler's draws in the trip."""
    sc, _, w, h = frames["44x27"]
    _same(*_both(_render(sc, B.camera(w, h, 0.6), w, h, 7)), "defocus 0.6")


def _launch(ds, cam, p, rows, w, stream=None):
    """One rt_launch, enqueued: (frame, counters) tensors."""
    import torch
    from rtclj._lib import check, lib
    out = torch.full((rows * w * 3,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    check(lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()),
                        C.c_void_p(stream.cuda_stream) if stream is not None else None))
    return out, cnt


@pytest.mark.parametrize("row_tile", [1, 8])
@pytest.mark.parametrize("name", sorted(B.FRAMES))
def test_interleaved_row_tiles(frames, name, row_tile):
    """tile_first = 1, tile_step = 2: the odd rows (a pool's eight rows two image
    rows apart) or the odd 8-row bands."""
    import torch
    from rtclj._lib import check, lib
    sc, cam, w, h = frames[name]
    ds = C.c_void_p()
    check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    try:
        p = B.params(w, h, spp=7, row_tile=row_tile, tile_first=1, tile_step=2)
        rows = lib.rt_rows_out(C.byref(p))
        assert rows > 0

        def go():
            out, cnt = _launch(ds, cam, p, rows, w)
            torch.cuda.synchronize()
            return out.cpu().numpy().reshape(rows, w, 3), tuple(cnt.cpu().tolist())
        _same(*_both(go), f"{name} row_tile {row_tile}")
    finally:
        lib.rt_scene_free(ds)


def test_two_streams(frames):
    """Both frames' scenes launched under the list on a stream each, nothing
    between the two launches: each equals its own launch under the walk."""
    import torch
    from rtclj._lib import check, lib
    jobs = []
    for name in sorted(B.FRAMES):
        sc, cam, w, h = frames[name]
        ds = C.c_void_p()
        check(lib.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
        jobs.append((name, ds, cam, B.params(w, h, spp=7), h, w, torch.cuda.Stream()))
    old = _variant(WALK)
    try:
        want = []
        for _, ds, cam, p, h, w, _ in jobs:
            out, cnt = _launch(ds, cam, p, h, w)
            torch.cuda.synchronize()
            want.append((out.cpu().numpy(), tuple(cnt.cpu().tolist())))
        _variant(LIST)
        got = [_launch(ds, cam, p, h, w, s) for _, ds, cam, p, h, w, s in jobs]
        torch.cuda.synchronize()
        for (name, *_), (fw, cw), (out, cnt) in zip(jobs, want, got):
            fl = out.cpu().numpy()
            assert np.array_equal(fl.view(np.uint32), fw.view(np.uint32)) and tuple(cnt.cpu().tolist()) == cw, name
    finally:
        lib.rt_set_variant(old)
        for _, ds, *_ in jobs:
            lib.rt_scene_free(ds)


def test_the_mirror(frames):
    """40 x 24, 7 spp under the list against the oracle's fp32 mirror."""
    from rtclj._lib import lib
    sc, cam, w, h = frames["40x24"]
    old = _variant(LIST)
    try:
        frame, (segs, _) = _render(sc, cam, w, h, 7, seed=5)()
    finally:
        lib.rt_set_variant(old)
    want, _, wsegs, _ = oracle.render(oracle.MODE_MIRROR32 | oracle.DIRECT, sc.sphere.astype(np.float64), sc.kind,
                                      sc.mat.astype(np.float64), cam.as_list(), cam.defocus, w, h, 7, DEPTH, seed=5)
    assert np.array_equal(frame, want) and segs == wsegs, "the list path against the fp32 mirror"


def test_statistics_build_counts_the_list_passes(frames):
    """Variant 31 renders 30's bits; rt_debug_stats_ext: a list pass tests four
    bodies or two (a pass's repeats included), an exact step belongs to a
    tested body: 2 passes <= bodies <= 4 passes, exact steps <= bodies."""
    from rtclj import raytracing as R
    from rtclj._lib import check, diag_lib
    d = diag_lib()
    sc, cam, w, h = frames["40x24"]
    got = {}
    old = d.rt_set_variant(WALK)
    assert old >= 0
    try:
        for v in (WALK, 31):
            assert d.rt_set_variant(v) >= 0, v
            check(d.rt_debug_stats((C.c_uint64 * 32)()))   # clear
            st = {}
            out = R.render(sc, cam, w, h, spp=7, max_depth=DEPTH, seed=3, n_devices=1, stats=st, library=d)
            dbg = (C.c_uint64 * 40)()
            check(d.rt_debug_stats_ext(dbg, 40))
            got[v] = (out, (st["segments"], st["samples"])), [int(x) for x in dbg]
    finally:
        d.rt_set_variant(old)
    _same(got[WALK][0], got[31][0], "variant 31")
    s = got[31][1]
    trips, lanes, passes, exacts, bodies = s[27], s[28], s[29], s[30], s[32]
    print(dict(trips=trips, lanes=lanes, passes=passes, exacts=exacts, bodies=bodies))
    assert trips > 0 and 0 < 2 * passes <= bodies <= 4 * passes and exacts <= bodies
    assert passes <= s[12] and exacts <= s[13] and all(x == 0 for x in s[33:])
    assert got[WALK][1][32] == 0
