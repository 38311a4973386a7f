"""The kernel's default path (loop-free samplers, flags = 0) against its
same-draw fp64 reference.

MODE_REF64 draws by the reference's rejection loops, so the default kernel's
paths are independent of its after the first scatter and the two compare only
statistically (oracle/pin.py BOUNDS_INDEPENDENT: a shading bias several times
the Monte-Carlo floor passes).  MODE_REF64D / MODE_REALM64D are the same fp64
path -- recursive ray-color, pow, division by a, un-normalised directions --
with the two samplers as their mathematical definition in plain double (z =
2 xi1 - 1 or r = sqrt(xi1), the angle 2 pi u / 2^24, libm cos and sin),
consuming the same uniforms as the kernel's sphere_direct / disk_direct.  The
paths then coincide except where an fp32 decision flips, and the kernel is held
to the same-draw BOUNDS (linear mean |d| <= 5e-4, 8-bit per-pixel mean <=
0.25, values off by > 1 <= 2 %, block means <= 0.25 / 2.5, segments per
sample within 2e-3), which a 1 % bias of the unit-sphere draw fails
(tests/test_oracle_cover_pin.py, test_oracle_pinning.py, test_realm.py).

Every test runs seed 1 and prints its statistics before it asserts; the
values measured on the MI355X stand in each docstring in the order
  seg_rel, lin_mean, px8_mean, px8_off_gt1, block_mean / block_max.
The bit-exact tests (test_gpu_parity.py, test_gpu_configs.py) already hold the
kernel to MODE_MIRROR32 | DIRECT, so these equal the CPU mirror's values.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from oracle.pin import BOUNDS, compare, within
from test_gpu_configs import _launch_rows, _oracle
from test_gpu_parity import variant

pytestmark = pytest.mark.gpu


def _launch_variant(dll, sc, w, h, spp, depth):
    """The variant a launch of this frame runs (rt_launch_occupancy)."""
    from rtclj._lib import check, rt_params
    ds = C.c_void_p()
    check(dll.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
    try:
        p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=depth, seed=1)
        o = (C.c_int * 4)()
        check(dll.rt_launch_occupancy(ds, C.byref(p), o))
        return o[3]
    finally:
        dll.rt_scene_free(ds)


def _hold(label, ref, segs, smp, img, segs32, smp32, by):
    assert ref.shape == img.shape and smp == smp32, (label, ref.shape, img.shape, smp, smp32)
    assert np.isfinite(img).all(), label
    st = compare(ref, segs / smp, img, segs32 / smp32, by=by)
    print(f"{label}: kernel (default samplers) vs fp64 same-draw reference: {st}")
    ok = within(st, BOUNDS)
    assert all(ok.values()), (label, ok, st)


def _frame(render, sc, cam, w, h, spp, depth, mode, label, by=9, library=None):
    st = {}
    g = render(sc, cam, w, h, spp=spp, max_depth=depth, seed=1, stats=st, flags=0, library=library)
    ref, segs, smp = _oracle(mode, sc, cam, w, h, spp, depth)
    _hold(label, ref, segs, smp, g, st["segments"], st["samples"], by)


def test_c0_against_ref64d(gpu_lib):
    """C0, the cover scene's whole frame, 200x112, 10 spp, depth 50; the
    default launch (variant 22, the compact image).
    Measured: 1.76e-4, 1.29e-4, 0.0353, 0.588 %, 0.0198 / 0.212."""
    from rtclj import raytracing as R
    from rtclj import scenes
    from rtclj._lib import lib
    sc = scenes.cover(11)
    assert _launch_variant(lib, sc, 200, 112, 10, 50) == 22
    _frame(R.render, sc, scenes.cover_camera(200, 112), 200, 112, 10, 50, oracle.MODE_REF64D, "C0")


def test_c1_rows_against_ref64d(gpu_lib):
    """C1, 1200x675, 100 spp, depth 50, every 32nd row (22 one-row tiles).
    Measured: 2.73e-4, 1.09e-4, 0.0293, 0.234 %, 0.00453 / 0.0206."""
    from rtclj import scenes
    sc = scenes.cover(11)
    w, h, spp = 1200, 675, 100
    cam = scenes.cover_camera(w, h)
    rows, segs32, smp32 = _launch_rows(sc, cam, w, h, spp, 50, row_tile=1, tile_first=0, tile_step=32, flags=0)
    ref, segs, smp = _oracle(oracle.MODE_REF64D, sc, cam, w, h, spp, 50, row_step=32)
    assert ref.shape == (22, w, 3)
    _hold("C1 rows", ref, segs, smp, rows, segs32, smp32, by=2)


def test_c4_kernel_against_ref64d(gpu_lib):
    """C4's own kernel -- 1000 bodies, depth 64, variant 26 (the compact
    4-body image, u8 stack, 1024-thread workgroups) -- on rows 0, 270, ...,
    4050 of the 7680x4320 frame at 16 spp (spp reduced from 2000 so that the
    fp64 path's linear scan over 1000 bodies takes seconds; the kernel's
    arithmetic does not depend on spp).
    Measured: 2.26e-4, 1.27e-4, 0.0367, 0.703 %, 0.00388 / 0.0258."""
    from rtclj import scenes
    from rtclj._lib import lib
    sc = scenes.cover_c4()
    w, h, spp, depth = 7680, 4320, 16, 64
    cam = scenes.cover_camera(w, h)
    assert _launch_variant(lib, sc, w, h, spp, depth) == 26
    rows, segs32, smp32 = _launch_rows(sc, cam, w, h, spp, depth, row_tile=1, tile_first=0, tile_step=270, flags=0)
    ref, segs, smp = _oracle(oracle.MODE_REF64D, sc, cam, w, h, spp, depth, row_step=270)
    assert ref.shape == (16, w, 3) and smp == 16 * w * spp
    _hold("C4 rows, variant 26", ref, segs, smp, rows, segs32, smp32, by=2)


def test_reference_scene_against_ref64d(gpu_lib):
    """The reference's own scene and camera, 400x225, 100 spp, depth 50.
    Measured: 1.57e-6, 2.49e-6, 6.85e-4, 0.00815 %, 5.3e-4 / 0.0128."""
    from rtclj import raytracing as R
    sc = R.Scene.from_bodies(R.hittables)
    cam = R.camera(400, 225, **R.REFERENCE_CAMERA)
    _frame(R.render, sc, cam, 400, 225, 100, 50, oracle.MODE_REF64D, "reference scene")


def test_reference_scene_realm_against_realm64d(gpu_lib):
    """The same frame with RT_FLAG_REALM (realm.raytracing's semantics; the
    camera's defocus disk draws too) against MODE_REALM64D.
    Measured: 2.66e-6, 2.25e-6, 6.78e-4, 0.00926 %, 5.0e-4 / 0.0288."""
    from rtclj import raytracing as R
    from rtclj import realm
    sc = R.Scene.from_bodies(R.hittables)
    cam = R.camera(400, 225, **R.REFERENCE_CAMERA)
    _frame(realm.render, sc, cam, 400, 225, 100, 50, oracle.MODE_REALM64D, "reference scene, realm")


def test_other_image_paths_against_ref64d(gpu_lib):
    """Not only the compact image: variant 16 (the 4-body walk on a u16 stack
    of LDS addresses, u64 sums) on C0, and variant 18 (the 8-body-leaf walk,
    u8 stack, the C4 scene's resolved variant) on the C4 scene framed at
    64x36, 16 spp, depth 64; selected as test_every_variant_is_bit_exact does.
    Measured: variant 16 as C0 above; variant 18: 2.56e-4, 1.12e-4, 0.0308,
    0.723 %, 0.0273 / 0.5."""
    from rtclj import raytracing as R
    from rtclj import scenes
    for v, sc, w, h, spp, depth in ((16, scenes.cover(11), 200, 112, 10, 50),
                                    (18, scenes.cover_c4(), 64, 36, 16, 64)):
        with variant(v) as dll:
            assert _launch_variant(dll, sc, w, h, spp, depth) == v
            _frame(R.render, sc, scenes.cover_camera(w, h), w, h, spp, depth, oracle.MODE_REF64D,
                   f"variant {v}, {w}x{h}", library=dll)
