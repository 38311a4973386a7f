"""rt_tile_bodies_host (include/rt.h): the camera prelude's list of one tile on
the host, csrc/tile_list.h's tl_host_tile -- the cull and the rectangle the
kernel's prologue takes, over the 4-body tree's leaf records.

lib/tile_bodies_check is tools/tile_list_check.cpp built under ASan and UBSan;
its `bodies` mode holds tl_host_tile to tile_keeps applied body by body over
random scenes and launches (every output a heap block of exactly its size, cap
below, at and above the count) and every entry to the body's and the index's
address.  lib/tile_list_check's C1 report gives the lists the benchmark's frame
runs with: 2.066 bodies a tile, 11 at most.  The rest calls the C entry on the
scenes of tests/test_gpu_body_list.py, whose tiles must hold every list length
the kernel can meet.
"""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "raytracing-clj_amd" / "lib"
sys.path.insert(0, str(Path(__file__).resolve().parent))

import body_list_scenes as B  # noqa: E402


def _run(exe, *args, timeout=120):
    assert exe.exists(), f"{exe} missing: run __graft_entry__.build()"
    p = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_host_entry_under_the_sanitizers():
    rep = _run(LIB / "tile_bodies_check", "bodies")
    print(rep)
    assert rep["bad"] == 0 and rep["tiles"] > 500 and rep["entries"] > 2000, rep
    assert rep["tiles_over_14"] > 0 and rep["tiles_empty"] > 0 and rep["interleaved_cases"] > 0, rep


def test_c1_histogram():
    """C1's 12,750 tiles by listed bodies: 11 at most, 2.066 a tile, none without a list."""
    c1 = _run(LIB / "tile_list_check", "1000")["c1"]
    hist = c1["tiles_by_bodies"]
    print(hist)
    assert sum(hist) == c1["tiles"] == 12750
    assert max(n for n, k in enumerate(hist) if k) == 11 == c1["max_bodies"]
    assert round(sum(n * k for n, k in enumerate(hist)) / 12750, 3) == 2.066 == c1["mean_bodies"]
    assert hist[0] / 12750 == pytest.approx(0.1475, abs=5e-5)
    assert sum(hist[:3]) > 0.7 * 12750   # (most tiles: one 2-body pass, or none)


def _rect(sc, cam, w, h, tile):
    """The tile's first and last pixel centres: columns, rows."""
    x0, y0 = 8 * (tile % ((w + 7) // 8)), 8 * (tile // ((w + 7) // 8))
    return x0, min(w, x0 + 8) - 1, y0, min(h, y0 + 8) - 1


@pytest.mark.parametrize("name", sorted(B.FRAMES))
def test_entry_equals_the_cull_body_by_body(name, tmp_path):
    """The C entry's count per tile = lib/tile_list_check count (tile_keeps over
    the scene's bodies, one by one); its bodies are distinct scene indices and
    its places distinct slots of the tree's records."""
    sc, cam, w, h = B.frame(name)
    lists = B.tile_lists(sc, cam, B.params(w, h))
    cam_line = " ".join(repr(float(np.float32(v))) for v in cam.as_list()) + f" {int(cam.defocus)}"
    body_lines = [" ".join(repr(float(v)) for v in b) for b in np.asarray(sc.sphere, np.float32)]
    for t, (bodies, slots) in enumerate(lists):
        x0, x1, y0, y1 = _rect(sc, cam, w, h, t)
        path = tmp_path / "tile.txt"
        path.write_text("\n".join([cam_line, f"{x0} {x1} {y0} {y1}"] + body_lines) + "\n")
        rep = _run(LIB / "tile_list_check", "count", str(path), timeout=30)
        assert rep == {"bodies": len(sc.sphere), "kept": len(bodies)}, (t, rep)
        assert len(set(bodies.tolist())) == len(bodies) and len(set(slots.tolist())) == len(slots)
        assert all(0 <= b < len(sc.sphere) for b in bodies) and all(0 <= s < 4 * len(sc.sphere) + 8 for s in slots)


def test_the_scenes_hold_every_list_length():
    """Over the GPU cases' frames: some tile lists exactly n bodies for every n
    in 0 .. 14, some tile 15 or more (no list: the walk); some list comes from
    one record, some from two at differing slots, some from five or more; and
    two listed bodies coincide."""
    got = [B.describe(B.tile_lists(*B.frame(name)[:2], B.params(*B.frame(name)[2:]))) for name in sorted(B.FRAMES)]
    print(got)
    assert set(range(15)) <= set().union(*(g["counts"] for g in got))
    for key in ("overflow", "one_record", "two_records", "five_records"):
        assert any(g[key] for g in got), key
    sc, cam, w, h = B.frame("40x24")
    twins = [t for t, (b, _) in enumerate(B.tile_lists(sc, cam, B.params(w, h)))
             if any(np.array_equal(sc.sphere[i], sc.sphere[j]) for i in b for j in b if i < j)]
    assert twins, "no tile lists two coincident bodies"


def test_interleaved_rows_and_bad_arguments():
    from rtclj._lib import lib, rt_params
    from rtclj import raytracing as R
    sc, cam, w, h = B.frame("40x24")
    # the odd 8-row bands: compacted tile row 0 is image rows 8 .. 15
    p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=1, max_depth=6, seed=1, row_tile=8, tile_first=1, tile_step=2)
    whole = B.tile_lists(sc, cam, B.params(w, h))
    band = B.tile_lists(sc, cam, p, rows=lib.rt_rows_out(C.byref(p)))
    assert len(band) == 5 and [b.tolist() for b, _ in band] == [b.tolist() for b, _ in whole[5:10]]
    # one-row tiles two rows apart: a pool's eight rows span fifteen image rows
    p1 = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=1, max_depth=6, seed=1, row_tile=1, tile_first=0, tile_step=2)
    wide = B.tile_lists(sc, cam, p1, rows=lib.rt_rows_out(C.byref(p1)))
    assert set(whole[0][0].tolist()) | set(whole[5][0].tolist()) <= set(wide[0][0].tolist())
    out = (C.c_int32 * 4)()
    assert lib.rt_tile_bodies_host(None, C.byref(cam), C.byref(p), 0, out, None, 4) < 0
    assert lib.rt_tile_bodies_host(C.byref(sc.c), C.byref(cam), C.byref(p), -1, out, None, 4) < 0
    assert lib.rt_tile_bodies_host(C.byref(sc.c), C.byref(cam), C.byref(p), 0, out, None, -1) < 0
    assert b"rt_tile_bodies_host" in lib.rt_last_error()
    assert lib.rt_tile_bodies_host(C.byref(sc.c), C.byref(cam), C.byref(p), 10 ** 6, out, None, 4) == 0   # (no pixels)
    assert R.tile_bodies_host(sc, cam, B.params(w, h), 14)[0].size == 14
