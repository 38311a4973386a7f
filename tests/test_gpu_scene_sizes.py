"""The refit, id and feature kernels on scenes above 1024 bodies
(tests/test_refit_host.py: LARGE -- cover(16), 1025 bodies; cover(46) cut to
2049; cover(46) cut to RT_MAX_SPHERES = 8192 with the body order permuted; the
random field of 8192).  There refit_kernel (csrc/bvh_refit.h) runs more than
one table workgroup, takes the second trip of its slot loop and, at 8192, of
its per-level node loop, and asks for more than 64 KB of dynamic LDS; the
feature and id passes read the tree from global memory on the policy's own
decision (csrc/variant_policy.h) and the path kernel falls back to variant 12.
Each test asserts those sizes from the trees the device holds
(check_size_edges).

Every comparison is on bits or integers against a witness that is not the
kernel under test: rt_tree_refit_host for the trees' bytes, a fresh upload for
frames after an update (the tables have no read-back), rt_ids_host for the ids,
the oracle's same-ray mirror for the features.  The checks themselves are
tests/test_gpu_refit.py's, tests/test_gpu_motion.py's and
tests/test_gpu_feat_oracle.py's.  All inputs are valid: nothing here can fault.
"""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_gpu_refit as G
from test_denoise_host import bits
from test_gpu_motion import device_ids
from test_refit_host import BODIES, EDGES, LARGE, THREADS, F, Tree, check_size_edges, scene

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
POLICY = ROOT / "raytracing-clj_amd" / "lib" / "variant_check"
W, H, SPP = 64, 36, 2
# variant_policy.h: kTraits' product rows with `lds` set, the tree (or the bodies) staged in LDS
LDS_RESIDENT = (16, 18, 22, 24, 26, 28)
FEAT_GLOBAL, FEAT_SCAN = 1, 2


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R, scenes
    e = Env()
    e.torch, e.R, e.scenes, e.lib = torch, R, scenes, gpu_lib.lib
    e.ds = None          # (test_gpu_feat's Feat)
    return e


def policy(infos, n, w, h, spp):
    """csrc/variant_policy.h applied to three rt_tree_infos and a frame, by
    lib/variant_check (the header built for the host; tests/test_variant_policy.py)
    -> {selector: (the variant a launch runs, the feature / id source)}."""
    import tempfile
    group = [0]
    for i in infos:
        group += [i.n_nodes, i.depth, i.blob_bytes // 16]
    group += [n, 1, w, h, h, spp, 0, 0]      # n_pad (unread for these variants), unit albedos, the frame, RTCLJ_TH4 unset
    with tempfile.NamedTemporaryFile("w", suffix=".json") as f:
        json.dump({"groups": [group]}, f)
        f.flush()
        out = subprocess.run([str(POLICY), f.name], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [[int(x) for x in line.split()] for line in out.stdout.splitlines()]
    return {r[1]: (r[3], r[8]) for r in rows if r[2] != -1}


def device_trees(d):
    """The three Trees of a DeviceScene, read back."""
    return [Tree(*d.tree(k)) for k in range(3)]


def visible_per_block(ids, n):
    """Per block of 1024 body indices, the distinct bodies a frame of ids shows."""
    seen = np.unique(ids[ids >= 0])
    return [int(((seen >= b) & (seen < b + THREADS)).sum()) for b in range(0, n, THREADS)]


# ---- 1. the device's bytes are the host refit's ------------------------------------------------
@pytest.mark.parametrize("name", LARGE)
def test_device_equals_host(env, name):
    """Upload == tree_build_host, the identity update, three updates on
    alternating streams == tree_refit_host, for the three trees.  After an
    8192-body update has raised the kernel's dynamic-LDS limit, a 484-body and a
    5-body scene in the same process still get the host's bytes."""
    up = G.check_device_equals_host(env, name)
    check_size_edges(name, [Tree(*t) for t in up])
    if "lds_above_64k" in EDGES[name]:
        for small, n in (("cover11", 484), ("reference", 5)):
            assert len(scene(small)) == n
            G.check_device_equals_host(env, small)


# ---- 2. the tables, through frames ---------------------------------------------------------------
@pytest.mark.parametrize("name", LARGE)
def test_frames_equal_a_fresh_upload(env, name):
    """geo, geo2 and sph have no read-back: the path frame under selectors 0,
    5 and 12, the feature pass and the ids (those also against ids_host) on the
    updated scene equal a fresh upload's, and the un-updated scene's differ.
    Every table workgroup's block of 1024 bodies shows in the frame (at least 5
    of them, or the block's all: the last block of cover16 and cover2049 holds
    one body); the linear scan (5) reads every body's entry for every ray."""
    R, lib = env.R, env.lib
    n = BODIES[name]
    sc0, sc1, camera = G.moving_pair(env, name)
    cam = camera(W, H)
    seen = visible_per_block(R.ids_host(sc1, cam, W, H), n)
    sizes = [min(THREADS, n - b) for b in range(0, n, THREADS)]
    assert len(seen) == len(sizes) >= 2 and all(s >= min(5, size) for s, size in zip(seen, sizes)), (name, seen)
    with R.DeviceScene(sc0) as d:
        check_size_edges(name, device_trees(d))
        want = policy([d.tree_info(k) for k in range(3)], n, W, H, SPP)
    ran = G.check_frames(env, name, W, H, (0, 5, 12), True, spp=SPP)
    assert ran == [want[0][0], 5, 12], (name, ran, want[0])
    if name == "cover2049":      # the slot loops stride while the path kernel still walks a tree in LDS
        assert ran[0] in LDS_RESIDENT, ran
    if "lds_above_64k" in EDGES[name]:
        assert ran[0] == 12, ran     # (tree too big for LDS: the policy's own fallback)


@pytest.mark.parametrize("name", LARGE)
def test_frames_of_the_diagnostic_library(env, name):
    G.check_diagnostic_frames(env, name)


# ---- 3. ordering at size ---------------------------------------------------------------------------
def test_update_is_ordered_on_its_stream(env):
    G.check_update_is_ordered(env, "cover8192")


# ---- 4. the pipeline ------------------------------------------------------------------------------
def test_render_animation_with_refit(env):
    """Three frames of cover(16) at 64 x 36: 30 visible field bodies and the
    last body (the second table workgroup's only one) rise 0.05 a frame; every
    stage of every frame with refit=True as without."""
    R = env.R
    sc = scene("cover16")
    cam = env.scenes.cover_camera(W, H)
    seen = np.unique(R.ids_host(sc, cam, W, H))
    field = seen[(seen >= 0) & (np.abs(sc.sphere[seen, 3]) < 1)][:30]
    assert len(field) == 30 and len(sc) - 1 in seen
    rising = np.r_[field, len(sc) - 1]
    seq = []
    for f in range(3):
        sph = sc.sphere.copy()
        sph[rising, 1] += F(0.05) * F(f)
        seq.append(G.with_spheres(env, sc, sph))
    cams = [cam] * 3
    plain = list(R.render_animation(seq, cams, W, H, spp=4, max_depth=G.DEPTH, seed=5, stages=True))
    refit = list(R.render_animation(seq, cams, W, H, spp=4, max_depth=G.DEPTH, seed=5, stages=True, refit=True))
    assert len(plain) == len(refit) == 3
    for f, (a, b) in enumerate(zip(plain, refit)):
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)), f
    assert not np.array_equal(plain[0][6], plain[2][6])      # (the motion shows in the ids)


# ---- 5. the id pass ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cover2049", "cover8192", "field8192"))
def test_ids_equal_host(env, name):
    """rt_launch_ids == rt_ids_host under selectors 0, 5, 12, 16, over three
    frame sizes and a row band, from the source the policy's text gives for the
    trees the device holds: the tree in global memory for 0, 12 and 16 (its
    image is beyond the LDS budget), the scan for 5."""
    R, lib = env.R, env.lib
    sc = scene(name)
    camera = G.scene_camera(env, name)
    out4 = (C.c_int * 4)()
    with R.DeviceScene(sc) as d:
        check_size_edges(name, device_trees(d))
        want_src = {sel: src for sel, (_, src) in policy([d.tree_info(k) for k in range(3)], len(sc), 65, 37, 1).items()}
        assert {sel: want_src[sel] for sel in (0, 5, 12, 16)} == {0: FEAT_GLOBAL, 5: FEAT_SCAN, 12: FEAT_GLOBAL, 16: FEAT_GLOBAL}
        for w, h in ((65, 37), (33, 17), (1, 1)):
            cam = camera(w, h)
            want = R.ids_host(sc, cam, w, h)
            for variant in (0, 5, 12, 16):
                old = lib.rt_set_variant(variant)
                try:
                    got = device_ids(env, d.handle, cam, w, h)
                    assert lib.rt_ids_occupancy(d.handle, out4) == 0
                finally:
                    lib.rt_set_variant(old)
                assert np.array_equal(got, want), (name, w, h, variant, int((got != want).sum()))
                assert out4[3] == want_src[variant] and out4[0] >= 1 and out4[1] > 0, (name, variant, tuple(out4))
            if (w, h) == (65, 37):
                assert len(np.unique(want)) > 50
                assert np.array_equal(device_ids(env, d.handle, cam, w, 12, row0=20), want[20:32])      # a row band
        assert lib.rt_set_variant(0) == 0


# ---- 6. the feature pass ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cover16", "cover8192"))
def test_features_equal_the_mirror(env, name):
    """rt_feat's sums, hits and depth bits against the oracle's same-ray
    mirror (tests/test_gpu_feat_oracle.py: _check) at 33 x 17, passes of 3 and 2
    samples from sample 5, the direct samplers.  The default selector's source
    is the tree in global memory here (1), where a small scene's is LDS (0)."""
    from test_gpu_feat_oracle import _check
    R = env.R
    sc = scene(name)
    infos = [R.tree_build_host(sc, k)[0] for k in range(3)]
    want = policy(infos, len(sc), 33, 17, 5)
    variants = tuple((sel, want[sel][1]) for sel in (0, 5, 12))
    assert variants == ((0, FEAT_GLOBAL), (5, FEAT_SCAN), (12, FEAT_GLOBAL))
    m = _check(env, sc, G.scene_camera(env, name)(33, 17), 33, 17, (3, 2), 9, begin=5, label=name, variants=variants)
    assert (m["hits"] > 0).mean() > 0.5 and m["sums"][..., 3:6].any()
