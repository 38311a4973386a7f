"""The fused budget trace's unit table on the host (include/rt.h:
rt_budget_units_host; csrc/budget.h's bd_units_at, the text
budget_units_kernel runs; no GPU needed): the table against a NumPy restatement
of rt.h's definition for random multipliers and any valid descending list; per
half exactly the set {(tile, 2 j + h) : j < mult[tile]}; block-major order, the
list's order within a block; the packed fields; a single tile, all ones and all
max_mult; the argument errors; the stand-alone sanitizer program; and the new
entries' declarations.
"""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_budget_host import tiles

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracing-clj_amd" / "lib" / "units_check"
FRAMES = ((9, 12), (33, 17), (64, 40))                        # width x height
NEW_FUNCS = ("rt_budget_trace_fused", "rt_budget_units_host", "rt_budget_units_read", "rt_budget_list_read")


def descending_list(mult, rng):
    """Any valid list: the tiles by descending multiplier, equal ones in random order."""
    perm = rng.permutation(mult.size)
    return perm[np.argsort(-mult[perm].astype(np.int64), kind="stable")].astype(np.int32)


def units_np(tile_list, mult, half, max_mult):
    """rt.h's definition: for pass j = 0 .. max_mult - 1 the list's tiles with
    mult > j, in list order; entry (tile, (2 j + half) | (2 max_mult) << 8)."""
    rows = [(t, (2 * j + half) | ((2 * max_mult) << 8)) for j in range(max_mult) for t in tile_list if mult[t] > j]
    return np.array(rows, np.int32).reshape(-1, 2)


def check_table(got, tile_list, mult, half, max_mult):
    want = units_np(tile_list, mult, half, max_mult)
    assert got.dtype == np.int32 and got.shape == want.shape == (int(mult.sum()), 2)
    assert np.array_equal(got, want)
    # the packed fields
    assert (got[:, 1] >> 8 == 2 * max_mult).all() and ((got[:, 1] & 255) <= 31).all()
    # as a set: exactly {(tile, 2 j + h) : j < mult[tile]}, no duplicates
    pairs = set(zip(got[:, 0].tolist(), (got[:, 1] & 255).tolist()))
    assert len(pairs) == len(got)
    assert pairs == {(t, 2 * j + half) for t in range(mult.size) for j in range(int(mult[t]))}
    # block-major; within a block the list's order
    k = got[:, 1] & 255
    assert (np.diff(k) >= 0).all() and (k % 2 == half).all()
    pos = np.empty(mult.size, np.int64)
    pos[tile_list] = np.arange(mult.size)
    for j in range(max_mult):
        block = got[k == 2 * j + half, 0]
        assert block.size == int((mult > j).sum()) and (np.diff(pos[block]) > 0).all()


@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("max_mult", (1, 4, 16))
def test_units_equal_the_definition(w, h, max_mult):
    from rtclj import raytracing as R
    gy, gx = tiles(h, w)
    rng = np.random.default_rng(100 * w + h + max_mult)
    for seed in range(3):
        mult = rng.integers(1, max_mult + 1, gy * gx).astype(np.uint32)
        tile_list = descending_list(mult, rng)
        keep = (tile_list.copy(), mult.copy())
        for half in (0, 1):
            got = R.budget_units_host(tile_list, mult, half, max_mult)
            check_table(got, tile_list, mult, half, max_mult)
        assert np.array_equal(tile_list, keep[0]) and np.array_equal(mult, keep[1])   # the inputs are never written
        # (gy, gx) multipliers, as Budget.mult gives them, are taken row-major
        assert np.array_equal(R.budget_units_host(tile_list, mult.reshape(gy, gx), 1, max_mult),
                              R.budget_units_host(tile_list, mult, 1, max_mult))


@pytest.mark.parametrize("max_mult", (1, 4, 16))
def test_units_edge_plans(max_mult):
    from rtclj import raytracing as R
    rng = np.random.default_rng(max_mult)
    one = np.zeros(1, np.int32)
    for m in (1, max_mult):                                   # a single tile
        for half in (0, 1):
            got = R.budget_units_host(one, np.full(1, m, np.uint32), half, max_mult)
            assert got.tolist() == [[0, (2 * j + half) | (2 * max_mult) << 8] for j in range(m)]
    n = 15                                                    # 33 x 17
    ones = np.ones(n, np.uint32)
    tile_list = descending_list(ones, rng)
    for half in (0, 1):
        got = R.budget_units_host(tile_list, ones, half, max_mult)
        assert len(got) == n and np.array_equal(got[:, 0], tile_list)        # U = n_tiles: the list itself
        check_table(got, tile_list, ones, half, max_mult)
        full = np.full(n, max_mult, np.uint32)
        got = R.budget_units_host(tile_list, full, half, max_mult)
        assert len(got) == n * max_mult and np.array_equal(got[:, 0], np.tile(tile_list, max_mult))
        check_table(got, tile_list, full, half, max_mult)
    # one tile at the cap, the rest 1 to 3: k up to 2 max_mult - 1
    mult = (1 + np.arange(n) % min(3, max_mult)).astype(np.uint32)
    mult[7] = max_mult
    tile_list = descending_list(mult, rng)
    got = R.budget_units_host(tile_list, mult, 1, max_mult)
    check_table(got, tile_list, mult, 1, max_mult)
    assert (got[-1] == (7, (2 * max_mult - 1) | (2 * max_mult) << 8)).all() or max_mult <= 3


def test_units_argument_errors():
    from rtclj._lib import i32ptr, lib, u32ptr
    from rtclj import raytracing as R
    mult = np.array([3, 1, 2, 3], np.uint32)
    good = np.array([0, 3, 2, 1], np.int32)
    out = np.full((9, 2), 77, np.int32)
    fn = lib.rt_budget_units_host
    assert fn(i32ptr(good), u32ptr(mult), 4, 3, 0, i32ptr(out)) == 9
    assert out.tolist() == [[0, 0 | 6 << 8], [3, 0 | 6 << 8], [2, 0 | 6 << 8], [1, 0 | 6 << 8],
                            [0, 2 | 6 << 8], [3, 2 | 6 << 8], [2, 2 | 6 << 8], [0, 4 | 6 << 8], [3, 4 | 6 << 8]]

    def refused(args, word):
        out[...] = 77
        assert fn(*args) == -1 and word in lib.rt_last_error(), (word, lib.rt_last_error())
        assert (out == 77).all()                              # nothing was written

    ok = [i32ptr(good), u32ptr(mult), 4, 3, 0, i32ptr(out)]
    for k in (0, 1, 5):
        refused(ok[:k] + [None] + ok[k + 1:], b"NULL")
    for n in (0, -4):
        refused(ok[:2] + [n] + ok[3:], b"n_tiles")
    for mm in (0, -1, 17):
        refused(ok[:3] + [mm] + ok[4:], b"max_mult")
    refused(ok[:3] + [2] + ok[4:], b"multiplier")             # a multiplier above max_mult
    refused([ok[0], u32ptr(np.array([3, 0, 2, 3], np.uint32))] + ok[2:], b"multiplier")
    for half in (-1, 2):
        refused(ok[:4] + [half] + ok[5:], b"half")
    for bad in ([1, 2, 0, 3], [0, 2, 3, 1], [3, 0, 1, 2]):    # ascending; one pair swapped; the 1 before the 2
        refused([i32ptr(np.array(bad, np.int32))] + ok[1:], b"descending")
    refused([i32ptr(np.array([0, 0, 2, 1], np.int32))] + ok[1:], b"twice")
    for bad in ([0, 3, 2, 4], [0, 3, 2, -1]):
        refused([i32ptr(np.array(bad, np.int32))] + ok[1:], b"outside")
    # the device entries refuse NULL handles before any device call
    assert lib.rt_budget_trace_fused(None, None, None, None, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_budget_units_read(None, 0, None, None) == -1 and b"NULL" in lib.rt_last_error()
    assert lib.rt_budget_list_read(None, None, None) == -1 and b"NULL" in lib.rt_last_error()
    # the Python layer
    with pytest.raises(R.RTError, match="descending"):
        R.budget_units_host([1, 2, 0, 3], mult, 0, 3)
    with pytest.raises(R.RTError, match="max_mult"):
        R.budget_units_host(good, mult, 0, 17)
    with pytest.raises(ValueError):
        R.budget_units_host(good[:3], mult, 0, 3)
    cam = R.camera(16, 9, **R.REFERENCE_CAMERA)
    with pytest.raises(TypeError):                            # `fused` is split off; the rest is still checked
        next(R.render_animation([R.hittables], [cam], 16, 9, budget=dict(half_spp=1, fused=True, tiles=3)))
    with pytest.raises(TypeError):
        next(R.render_animation([R.hittables], [cam], 16, 9, budget=dict(fused=True)))


def test_units_check_runs_clean():
    """tools/units_check.cpp: the host table under AddressSanitizer and
    UndefinedBehaviorSanitizer, every array a heap block of exactly its size."""
    assert TOOL.exists(), f"{TOOL} is missing (make -C raytracing-clj_amd)"
    out = subprocess.run([str(TOOL)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["entries"] > 100000 and rep["calls"] > 100


def test_new_entries_are_declared_bound_and_cited():
    from rtclj._lib import ADDITIVE, SIGNATURES, lib
    from rtclj import raytracing as R
    header = (ROOT / "include" / "rt.h").read_text()
    section = header[header.index("the sample budget: samples where"):header.index("an uploaded scene updated in place")]
    for name in NEW_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, section), name
        assert name in SIGNATURES and name in ADDITIVE and hasattr(lib, name), name
    fused = section[section.index("int rt_budget_trace("):section.index("int rt_budget_trace_fused(")]
    assert "raytracing.clj:141-155" in fused and "not the bits" in fused
    assert "budget_units_host" in R.__all__ and hasattr(R.Budget, "units")
    assert "fused" in R.Budget.trace.__code__.co_varnames
