"""What tests/test_gpu_list_modes.py relies on, held on the host: the frames of
tests/body_list_scenes.py in which every launch mode of the path kernel is run
have a list in nearly every tile, as rt_tile_bodies_host (include/rt.h) counts
it, and the refit case's moved scene changes lists without changing what
rt_scene_update needs unchanged.  These are conditions on the scenes, not
measurements: they hold by construction of staircase.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import body_list_scenes as B  # noqa: E402


def _counts(sc, cam, w, h):
    return [len(b) for b, _ in B.tile_lists(sc, cam, B.params(w, h))]


def test_every_whole_tile_of_40x24_is_listed():
    sc, cam, w, h = B.frame("40x24")
    counts = _counts(sc, cam, w, h)
    assert counts == list(range(15))
    assert B.listed_tiles(sc, cam, B.params(w, h)) == list(range(15))
    assert sum(1 for c in counts if 1 <= c <= 14) >= 14


def test_the_frame_with_partial_tiles_lists_most_and_overflows_some():
    sc, cam, w, h = B.frame("44x27m")
    counts = _counts(sc, cam, w, h)
    print(counts)
    assert len(counts) == 24
    listed = B.listed_tiles(sc, cam, B.params(w, h))
    assert listed == [t for t, c in enumerate(counts) if c <= 14]
    assert sum(1 for t in listed if counts[t] >= 1) >= 14
    assert sum(1 for c in counts if c > 14) >= 8
    # the partial tiles (last column, last row) on both sides of the limit
    partial = [t for t in range(24) if t % 6 == 5 or t // 6 == 3]
    assert any(1 <= counts[t] <= 14 for t in partial) and any(counts[t] > 14 for t in partial)
    # the budget case's tiles: these exact lengths, and an overflowed tile
    assert [counts[t] for t in (0, 1, 2, 3, 9)] == [0, 1, 2, 5, 14] and counts[12] > 14
    # lists out of five leaf records and more
    assert B.describe(B.tile_lists(sc, cam, B.params(w, h)))["five_records"]


def test_the_existing_frames_are_unchanged():
    """staircase's new arguments leave the frames of tests/test_gpu_body_list.py as they were."""
    sc, cam, w, h = B.frame("44x27")
    assert len(sc) == 260 and _counts(sc, cam, w, h)[:4] == [0, 1, 2, 3]
    assert len(B.frame("40x24")[0]) == 98


def test_moved_changes_lists_and_nothing_an_update_cannot_follow():
    from rtclj import raytracing as R
    sc, cam, w, h = B.frame("40x24")
    before = _counts(sc, cam, w, h)
    own = [int((sc.stair["body"][:, 0] == t).sum()) for t in range(15)]   # a tile's small spheres
    for k, overflow in ((0, [13]), (1, [11, 14]), (2, [9, 12])):
        mv = B.moved(sc, k)
        tiles = B.moved_tiles(sc, k)
        assert tiles == [t for t in range(15) if t % 3 == k and own[t]]
        # by construction: a moved tile keeps its big bodies; the next tile of
        # its row receives its spheres (a row's last tile, t % 5 == 4, sends them
        # out of the frame); nothing else changes
        want = list(before)
        for t in tiles:
            want[t] -= own[t]
            if t % 5 != 4:
                want[t + 1] += own[t]
        after = _counts(mv, cam, w, h)
        assert after == want, (k, after, want)
        assert sum(1 for a, b in zip(before, after) if a != b) >= 4
        # which tiles have no list, before and after: none, then exactly these
        assert [t for t, c in enumerate(before) if c > 14] == []
        assert [t for t, c in enumerate(after) if c > 14] == overflow, k
        # rt_scene_update's condition: the same bodies but for their centres, so
        # the upload's trees keep their topology and the host refit accepts them
        assert R._same_but_centres(sc, mv) and np.isfinite(mv.sphere).all()
        assert not np.array_equal(mv.sphere, sc.sphere)
        big = sc.stair["body"][:, 0] < 0
        assert np.array_equal(mv.sphere[big], sc.sphere[big])
        for tree in range(3):
            info, blob = R.tree_build_host(sc, tree)
            info2, blob2 = R.tree_refit_host(info, blob, sc, mv)
            assert blob2.size == blob.size and not np.array_equal(blob2, blob)
            a, b = info.as_dict(), info2.as_dict()
            for key in ("n_nodes", "off_pairs", "off_pidx", "blob_bytes", "big_pair0", "n_big_leaves", "depth",
                        "leaf_size", "idx_bytes"):
                assert a[key] == b[key], (tree, key)
            # and back: the original scene's bytes again
            _, blob3 = R.tree_refit_host(info2, blob2, mv, sc)
            assert np.array_equal(blob3, blob), tree
