"""Refitting a scene's trees on the device (include/rt.h: rt_scene_update,
rt_scene_tree_info, rt_scene_tree_read): after an update the device holds
rt_tree_refit_host's bytes, for the host tests' scenes and motions, three
updates in a row, on the NULL stream and a stream of its own; a frame traced on
the updated scene equals, bit for bit, the frame on a scene freshly uploaded
from the moved spheres, for every product variant, the feature pass and the
body ids (those also against ids_host: a witness that is not the device), with
the frame of the un-updated scene as the control; stream order; the errors;
and render_animation(refit=True).  Every output buffer is pre-filled (floats
with NaN, ids with 0x7fffffff).  All inputs are valid: nothing here can fault.  The checks
are functions (check_*) that tests/test_gpu_scene_sizes.py runs again on the
scenes above 1024 bodies.
"""
import ctypes as C

import numpy as np
import pytest

from test_denoise_host import bits
from test_motion_host import rising
from test_refit_host import MOTIONS, SCENES, F, moved, scene

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 36, 4, 8
FILL = 0x7fffffff
VARIANTS = (0, 5, 12, 16, 22, 18)


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    from rtclj import raytracing as R, scenes
    e = Env()
    e.torch, e.R, e.scenes, e.lib = torch, R, scenes, gpu_lib.lib
    return e


def params(env, w, h, spp=SPP, depth=DEPTH):
    from rtclj._lib import rt_params
    return rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=depth, seed=3)


def enqueue_frame(env, lib, ds, cam, w, h, stream=None, spp=SPP):
    """rt_launch into a NaN-filled buffer, not waited for."""
    torch = env.torch
    d = torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = params(env, w, h, spp)
    st = C.c_void_p(stream.cuda_stream) if stream is not None else None
    assert lib.rt_launch(ds, C.byref(cam), C.byref(p), C.c_void_p(d.data_ptr()), None, st) == 0, lib.rt_last_error()
    return d


def frame(env, lib, ds, cam, w, h, stream=None, spp=SPP):
    d = enqueue_frame(env, lib, ds, cam, w, h, stream, spp)
    env.torch.cuda.synchronize()
    got = d.cpu().numpy().reshape(h, w, 3)
    assert not np.isnan(got).any()
    return got


def feat_frame(env, ds, cam, w, h):
    """rt_launch_feat of SPP samples, resolved -> (h, w, 8)."""
    from rtclj._lib import RT_FEAT_CHANNELS
    torch, lib = env.torch, env.lib
    d = torch.full((w * h * RT_FEAT_CHANNELS,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = params(env, w, h, depth=1)
    ft = C.c_void_p()
    assert lib.rt_feat_create(ds, C.byref(p), C.byref(ft)) == 0, lib.rt_last_error()
    try:
        assert lib.rt_launch_feat(ds, C.byref(cam), C.byref(p), ft, None, None) == 0, lib.rt_last_error()
        assert lib.rt_feat_resolve(ft, C.c_void_p(d.data_ptr()), None) == 0, lib.rt_last_error()
        torch.cuda.synchronize()
    finally:
        lib.rt_feat_free(ft)
    return d.cpu().numpy().reshape(h, w, RT_FEAT_CHANNELS)


def ids_frame(env, ds, cam, w, h):
    torch = env.torch
    d = torch.full((w * h,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert env.lib.rt_launch_ids(ds, C.byref(cam), w, h, 0, C.c_void_p(d.data_ptr()), None) == 0, env.lib.rt_last_error()
    torch.cuda.synchronize()
    got = d.cpu().numpy().reshape(h, w)
    assert not (got == FILL).any()
    return got


def with_spheres(env, sc, sph):
    return env.R.Scene(sph, sc.kind, sc.mat)


# ---- 1. the device's bytes are the host refit's ------------------------------------------------
def check_device_equals_host(env, name):
    """-> the three trees (info, blob) as the upload left them on the device."""
    R = env.R
    sc = scene(name)
    own = env.torch.cuda.Stream()
    with R.DeviceScene(sc) as d:
        up = [d.tree(k) for k in range(3)]
        for k in range(3):     # what was uploaded is what the host builds
            info, blob = R.tree_build_host(sc, k)
            assert bytes(up[k][0]) == bytes(info) and up[k][1].tobytes() == blob.tobytes(), (name, k)
        d.update(sc)           # the identity: every byte as read before it
        for k in range(3):
            info, blob = d.tree(k)
            assert bytes(info) == bytes(up[k][0]) and blob.tobytes() == up[k][1].tobytes(), (name, k)
        for step, motion in enumerate(MOTIONS):      # three updates in a row, the streams alternating
            sph = moved(name, motion)
            stream = own.cuda_stream if step % 2 else None
            d.update(sph, stream=stream)
            for k in range(3):
                info, blob = d.tree(k, stream=stream)
                want_info, want = R.tree_refit_host(up[k][0], up[k][1], sc, sph)
                assert blob.tobytes() == want.tobytes(), (name, motion, k, int((blob != want).sum()))
                assert bytes(info) == bytes(want_info), (name, motion, k)
    return up


@pytest.mark.parametrize("name", SCENES)
def test_device_equals_host(env, name):
    check_device_equals_host(env, name)


# ---- 2. rendered frames ------------------------------------------------------------------------------
def moving_pair(env, which):
    R = env.R
    if which == "reference":
        return (R.Scene.from_bodies(rising(0, 4)), R.Scene.from_bodies(rising(3, 4)),
                lambda w, h: R.camera(w, h, **R.REFERENCE_CAMERA))
    sc = scene(which)
    return sc, with_spheres(env, sc, moved(which, "jitter")), scene_camera(env, which)


def scene_camera(env, which):
    """(w, h) -> the camera of a scene of tests/test_refit_host.py: the cover
    scene's, or for the random field test_max_spheres_and_too_many's."""
    if which.startswith("field"):
        return lambda w, h: env.R.camera(w, h, 40.0, (0, 1, 3), (0, 1, -10), (0, 1, 0), 0.0, 10.0)
    return env.scenes.cover_camera


def check_frames(env, which, w, h, variants, everything, spp=SPP):
    """-> the variants that ran (rt_launch_occupancy), in `variants`' order."""
    R, lib = env.R, env.lib
    sc0, sc1, camera = moving_pair(env, which)
    cam = camera(w, h)
    out4 = (C.c_int * 4)()
    with R.DeviceScene(sc0) as old, R.DeviceScene(sc0) as upd, R.DeviceScene(sc1) as new:
        upd.update(sc1)
        ran = []
        for variant in variants:
            before = lib.rt_set_variant(variant)
            try:
                p = params(env, w, h, spp)
                assert lib.rt_launch_occupancy(upd.handle, C.byref(p), out4) == 0
                ran.append(out4[3])
                got = frame(env, lib, upd.handle, cam, w, h, spp=spp)
                want = frame(env, lib, new.handle, cam, w, h, spp=spp)
                assert np.array_equal(bits(got), bits(want)), (which, variant, out4[3], int((got != want).any(axis=-1).sum()))
                if variant == 0:
                    # the control: the motion shows, so a refit that did nothing would
                    stale = frame(env, lib, old.handle, cam, w, h, spp=spp)
                    assert int((stale != want).any(axis=-1).sum()) > 20
                if everything and variant in (0, 5, 12):      # the feature pass and the ids under each source of bodies
                    assert np.array_equal(bits(feat_frame(env, upd.handle, cam, w, h)), bits(feat_frame(env, new.handle, cam, w, h)))
                    ids = ids_frame(env, upd.handle, cam, w, h)
                    assert np.array_equal(ids, ids_frame(env, new.handle, cam, w, h)), (which, variant)
                    assert np.array_equal(ids, R.ids_host(sc1, cam, w, h)), (which, variant)
                    if variant == 0:
                        assert not np.array_equal(ids, ids_frame(env, old.handle, cam, w, h))
            finally:
                lib.rt_set_variant(before)
    assert lib.rt_set_variant(0) == 0
    return ran


@pytest.mark.parametrize("which", ("reference", "cover"))
def test_frames_equal_a_fresh_upload(env, which):
    ran = set(check_frames(env, which, W, H, VARIANTS, True))
    # (the policy may run 16 as its compact image 22, and 18 as 24 or 26)
    assert {5, 12} <= ran and ran & {16, 22} and ran & {18, 24, 26}, ran


def test_frames_of_a_larger_scene(env):
    """cover(11): 484 bodies, trees of several levels, at 65 x 37."""
    assert len(scene("cover11")) == 484
    check_frames(env, "cover11", 65, 37, (0, 18), False)


def test_frames_of_the_diagnostic_library(env):
    check_diagnostic_frames(env, "cover")


def check_diagnostic_frames(env, which):
    """Variant 9 reads the pair-interleaved table (geo2)."""
    from rtclj._lib import diag_lib
    R = env.R
    d = diag_lib()
    sc0, sc1, camera = moving_pair(env, which)
    cam = camera(W, H)
    before = d.rt_set_variant(9)
    assert before >= 0
    try:
        with R.DeviceScene(sc0, library=d) as upd, R.DeviceScene(sc1, library=d) as new:
            stale = frame(env, d, upd.handle, cam, W, H)
            upd.update(sc1)
            got, want = frame(env, d, upd.handle, cam, W, H), frame(env, d, new.handle, cam, W, H)
            assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(stale), bits(want))
    finally:
        d.rt_set_variant(before)


# ---- 3. ordering --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("reference", "cover"))
def test_update_is_ordered_on_its_stream(env, which):
    check_update_is_ordered(env, which)


def check_update_is_ordered(env, which):
    """Launch A, the update, launch B on one stream with nothing in between,
    and the caller's array overwritten as soon as the update returns."""
    from rtclj._lib import fptr
    R, lib = env.R, env.lib
    sc0, sc1, camera = moving_pair(env, which)
    cam = camera(W, H)
    with R.DeviceScene(sc0) as old, R.DeviceScene(sc1) as new:
        want_a, want_b = frame(env, lib, old.handle, cam, W, H), frame(env, lib, new.handle, cam, W, H)
    assert not np.array_equal(bits(want_a), bits(want_b))
    stream = env.torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    mine = sc1.sphere.copy()
    with R.DeviceScene(sc0) as d:
        a = enqueue_frame(env, lib, d.handle, cam, W, H, stream)
        assert lib.rt_scene_update(d.handle, fptr(mine), st) == 0, lib.rt_last_error()
        mine[...] = np.nan
        b = enqueue_frame(env, lib, d.handle, cam, W, H, stream)
        env.torch.cuda.synchronize()
        assert np.array_equal(bits(a.cpu().numpy().reshape(H, W, 3)), bits(want_a))
        assert np.array_equal(bits(b.cpu().numpy().reshape(H, W, 3)), bits(want_b))


# ---- 4. errors ---------------------------------------------------------------------------------------------
def test_errors_change_nothing(env):
    from rtclj._lib import RT_E_ARG, fptr
    R, lib = env.R, env.lib
    sc = scene("cover")
    cam = env.scenes.cover_camera(W, H)
    sph = moved("cover", "jitter")
    with R.DeviceScene(sc) as d:
        d.update(sph)
        want = frame(env, lib, d.handle, cam, W, H)
        trees = [d.tree(k) for k in range(3)]
        assert lib.rt_scene_update(None, fptr(sph), None) == RT_E_ARG
        assert lib.rt_scene_update(d.handle, None, None) == RT_E_ARG and b"NULL" in lib.rt_last_error()
        bad = sph.copy()
        bad[7, 3] = np.nextafter(bad[7, 3], F(np.inf))
        assert lib.rt_scene_update(d.handle, fptr(bad), None) == RT_E_ARG and b"radius" in lib.rt_last_error()
        bad = sph.copy()
        bad[7, 1] = np.nan
        assert lib.rt_scene_update(d.handle, fptr(bad), None) == RT_E_ARG and b"finite" in lib.rt_last_error()
        with pytest.raises(ValueError):
            d.update(sph[:-1])
        for k in range(3):
            info, blob = d.tree(k)
            assert bytes(info) == bytes(trees[k][0]) and blob.tobytes() == trees[k][1].tobytes()
        assert np.array_equal(bits(frame(env, lib, d.handle, cam, W, H)), bits(want))
        assert lib.rt_scene_tree_info(d.handle, 3, C.byref(trees[0][0])) == RT_E_ARG
        short = np.zeros(trees[0][0].blob_bytes - 1, np.uint8)
        assert lib.rt_scene_tree_read(d.handle, 0, short.ctypes.data_as(C.c_void_p), short.size, None) == RT_E_ARG
    # a scene of no body: nothing to move
    empty = R.Scene(np.zeros((0, 4), F), np.zeros(0, np.int32), np.zeros((0, 4), F))
    with R.DeviceScene(empty) as d:
        before = [d.tree(k)[1].tobytes() for k in range(3)]
        assert lib.rt_scene_update(d.handle, None, None) == 0
        assert [d.tree(k)[1].tobytes() for k in range(3)] == before


# ---- 5. the pipeline ---------------------------------------------------------------------------------------
def test_render_animation_with_refit(env):
    """Four frames of the rising sphere at 64 x 36: every stage of every frame
    as without the keyword; and with a third frame whose radius differs, which
    neither rt_scene_update nor the frame after it can reach by an update."""
    R = env.R
    cams = []
    for f in range(4):      # test_gpu_temporal's 0.4-degree orbit, at this frame size
        ang = np.radians(0.4) * f
        lf = (-2.0 * np.cos(ang) + 1.0 * np.sin(ang), 2.0, 2.0 * np.sin(ang) + 1.0 * np.cos(ang))
        cams.append(R.camera(W, H, **{**R.REFERENCE_CAMERA, "look_from": lf}))
    scs = [R.Scene.from_bodies(rising(f, 4)) for f in range(4)]
    odd = [R.Scene.from_bodies(rising(f, 4)) for f in range(4)]
    odd[2].sphere[1, 3] = 0.45
    for seq in (scs, odd):
        plain = list(R.render_animation(seq, cams, W, H, spp=4, max_depth=DEPTH, seed=5, stages=True))
        refit = list(R.render_animation(seq, cams, W, H, spp=4, max_depth=DEPTH, seed=5, stages=True, refit=True))
        assert len(plain) == len(refit) == 4
        for f, (a, b) in enumerate(zip(plain, refit)):
            for x, y in zip(a, b):
                assert np.array_equal(bits(x), bits(y)), f
    assert not np.array_equal(bits(plain[2][0]), bits(list(R.render_animation(scs[:3], cams[:3], W, H, spp=4, max_depth=DEPTH, seed=5))[2]))
