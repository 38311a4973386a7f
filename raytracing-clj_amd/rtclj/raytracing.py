"""Mirror of src/raytracing.clj — the reference's host entry points.

    hittables       raytracing.clj:63-78   the five-body scene, as data
    camera          raytracing.clj:105-139 basis/viewport (rt_camera_setup)
    render          raytracing.clj:141-171 compute-pixel over every pixel,
                                           on the GPU(s) via rt_render
    write_color     raytracing.clj:19-26   gamma-2, clamp 0.999, x256
    write_ppm       raytracing.clj:172-175 P3, one pixel per line
    write_png,      ppm2png.clj:35-87      8-bit RGB PNG of the same pixels
      ppm_to_png
    main            raytracing.clj:95-177  `clojure -M:main [spp] [depth]`

The per-pixel loop (compute-pixel -> ray-color -> hit-anything -> hit-fn /
scatter-fn) is the hand-written gfx950 kernel behind include/rt.h.  There is
no CPU path here: without the library or a GPU, render raises RTError.
"""
from __future__ import annotations

import ctypes as C
import sys
import time
from fractions import Fraction

import numpy as np

from . import hittable, material
from ._lib import (BUDGET_DEFAULTS, DENOISE_DEFAULTS, RT_DIELECTRIC, RT_FEAT_CHANNELS, RT_LAMBERTIAN, RT_METAL, RT_NONE,
                   TEMPORAL_CLAMP_DEFAULTS, TEMPORAL_DEFAULTS, RTError, check, dptr, fptr, i64ptr, iptr, lib,
                   rt_adapt_opts, rt_budget_opts, rt_camera, i32ptr, rt_denoise_opts, rt_params, rt_scene, rt_schedule_info, rt_stats,
                   rt_temporal_clamp_opts, rt_temporal_opts, rt_tree_info, u8ptr, u32ptr, u64ptr,
                   UPSAMPLE_DEFAULTS, rt_upsample_opts, CHAIN_DEFAULTS, CHAIN_SAMPLE_DTYPE, rt_chain_sample,
                   rt_feat_chain_opts, RAY_DTYPE, RAY_HIT_DTYPE, rt_ray, rt_ray_hit)

# ---- scene (raytracing.clj:63-78) --------------------------------------------
hittables = [
    {**hittable.sphere((0.0, -100.5, -1.0), 100.0), **material.lambertian((0.8, 0.8, 0.0))},   # ground
    {**hittable.sphere((0.0, 0.0, -1.2), 0.5), **material.lambertian((0.1, 0.2, 0.5))},       # center
    {**hittable.sphere((-1.0, 0.0, -1.0), 0.5), **material.dielectric(1.5)},                  # left
    {**hittable.sphere((-1.0, 0.0, -1.0), 0.4), **material.dielectric(1.00 / 1.5)},          # bubble
    {**hittable.sphere((1.0, 0.0, -1.0), 0.5), **material.metal((0.8, 0.6, 0.2), 1.0)},       # right
]

# camera constants of -main (raytracing.clj:105-115)
ASPECT = Fraction(16, 9)
REFERENCE_CAMERA = dict(vfov=20.0, look_from=(-2.0, 2.0, 1.0), look_at=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0),
                        defocus_angle=10.0, focus_dist=3.4)


def image_height(image_width: int, aspect=ASPECT) -> int:
    """(int (/ image-width aspect-ratio)) with Clojure's exact ratio (:105-107)."""
    return int(Fraction(image_width) / Fraction(aspect))


def flatten(bodies):
    """Bodies (merged hittable+material maps) -> the rt_scene arrays.

    Returns (sphere float32[n,4], kind int32[n], mat float32[n,4]).  A body
    with no material is kept (it renders black, as ray-color does when the hit
    body has no ::scatter-fn, raytracing.clj:49-54)."""
    n = len(bodies)
    sph = np.zeros((n, 4), np.float32)
    kind = np.zeros(n, np.int32)
    mat = np.zeros((n, 4), np.float32)
    for i, b in enumerate(bodies):
        if b.get("hittable/kind") != "sphere":
            raise ValueError(f"body {i}: only spheres are supported (hittable.clj:7)")
        sph[i, :3] = b["hittable/center"]
        sph[i, 3] = b["hittable/radius"]
        t = b.get("material/type")
        if t == "lambertian":
            kind[i] = RT_LAMBERTIAN
            mat[i, :3] = b["material/albedo"]
        elif t == "metal":
            kind[i] = RT_METAL
            mat[i, :3] = b["material/albedo"]
            mat[i, 3] = b["material/fuzz"]
        elif t == "dielectric":
            kind[i] = RT_DIELECTRIC
            mat[i, 3] = b["material/refraction-index"]
        elif t is None:
            kind[i] = RT_NONE
        else:
            raise ValueError(f"body {i}: unsupported material {t!r}")
    return sph, kind, mat


def flatten64(bodies):
    """As flatten, in float64 (the oracle's reference-semantics input)."""
    sph, kind, mat = flatten(bodies)
    sph64 = np.array([[*b["hittable/center"], b["hittable/radius"]] for b in bodies], np.float64).reshape(-1, 4)
    mat64 = np.zeros((len(bodies), 4), np.float64)
    for i, b in enumerate(bodies):
        if "material/albedo" in b:
            mat64[i, :3] = b["material/albedo"]
        mat64[i, 3] = b.get("material/fuzz", b.get("material/refraction-index", 0.0))
    return sph64, kind, mat64


class Scene:
    """Flattened scene arrays plus the rt_scene struct pointing at them."""

    def __init__(self, sphere, kind, mat):
        self.sphere = np.ascontiguousarray(sphere, np.float32).reshape(-1, 4)
        self.kind = np.ascontiguousarray(kind, np.int32).reshape(-1)
        self.mat = np.ascontiguousarray(mat, np.float32).reshape(-1, 4)
        if not (len(self.sphere) == len(self.kind) == len(self.mat)):
            raise ValueError("scene arrays disagree in length")
        self.c = rt_scene(len(self.kind), fptr(self.sphere), iptr(self.kind), fptr(self.mat))

    @classmethod
    def from_bodies(cls, bodies):
        return cls(*flatten(bodies))

    def __len__(self):
        return len(self.kind)


def camera(image_width, image_h, vfov, look_from, look_at, vup, defocus_angle, focus_dist) -> rt_camera:
    """Camera values of -main (raytracing.clj:117-139), computed in double."""
    cam = rt_camera()
    d3 = C.c_double * 3
    check(lib.rt_camera_setup(int(image_width), int(image_h), float(vfov), d3(*look_from), d3(*look_at),
                              d3(*vup), float(defocus_angle), float(focus_dist), C.byref(cam)))
    return cam


def _frame_args(scene, width, height, spp, max_depth, seed, n_devices, rows, sample_begin, row_tile, flags, out, u8):
    if not isinstance(scene, Scene):
        scene = Scene.from_bodies(scene)
    r0, r1 = (0, height) if rows is None else rows
    p = rt_params(width=width, height=height, row_begin=r0, row_end=r1, spp=spp, max_depth=max_depth,
                  seed=seed, sample_begin=sample_begin, n_devices=n_devices, row_tile=row_tile, flags=flags)
    shape = (max(r1 - r0, 0), width, 3)
    dt = np.uint8 if u8 else np.float32
    if out is None:
        out = np.empty(shape, dt)
    elif out.shape != shape or out.dtype != dt or not out.flags.c_contiguous:
        raise ValueError(f"render: out must be C-contiguous {np.dtype(dt).name} {shape}")
    return scene, p, out


class Progressive:
    """compute-pixel's sample loop (raytracing.clj:141-155) continued across
    launches: a frame whose samples are added pass by pass on device `device`
    (rt_accum, include/rt.h).  After any passes, frame() is bit for bit the
    frame one launch of `samples` spp gives.

        pr = Progressive(scene, cam, 400, 225)
        pr.add(8); show(pr.frame_u8())       # 8 spp now
        pr.add(24); show(pr.frame_u8())      # the 32-spp frame, refined

    add() advances sample_begin itself.  `stream`: a HIP stream handle (int)
    for the passes and copies, default the NULL stream.  frame(), frame_u8()
    and sums() wait for the passes enqueued on it."""

    def __init__(self, scene, cam: rt_camera, width: int, height: int, max_depth: int = 50, seed: int = 1,
                 rows=None, row_tile: int = 8, tile_first: int = 0, tile_step: int = 0, flags: int = 0,
                 sample_begin: int = 0, device: int = 0, stream=None, library=None):
        self._dll = library if library is not None else lib
        self.scene = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
        self.cam = cam
        r0, r1 = (0, height) if rows is None else rows
        self._p = rt_params(width=width, height=height, row_begin=r0, row_end=r1, spp=0, max_depth=max_depth,
                            seed=seed, sample_begin=sample_begin, row_tile=row_tile, tile_first=tile_first,
                            tile_step=tile_step, flags=flags)
        self._first, self._next = sample_begin, sample_begin
        self._stream = C.c_void_p(stream) if stream else None
        self._ds, self._acc = C.c_void_p(), C.c_void_p()
        self._check(self._dll.rt_scene_upload(int(device), C.byref(self.scene.c), C.byref(self._ds)))
        try:
            self._check(self._dll.rt_accum_create(self._ds, C.byref(self._p), C.byref(self._acc)))
        except RTError:
            self.close()
            raise
        self.shape = (self._dll.rt_rows_out(C.byref(self._p)), width, 3)

    def _check(self, code):
        if code < 0:
            raise RTError(code, self._dll.rt_last_error().decode(errors="replace"))
        return code

    @property
    def samples(self) -> int:
        """Samples per pixel added so far (rt_accum_samples)."""
        return int(self._dll.rt_accum_samples(self._acc))

    def add(self, spp: int) -> int:
        """Enqueue one pass of `spp` more samples per pixel (rt_launch_accum);
        returns the new count."""
        if spp < 0:
            raise ValueError("Progressive.add: spp < 0")
        self._p.spp = int(spp)
        self._p.sample_begin = self._next
        self._check(self._dll.rt_launch_accum(self._ds, C.byref(self.cam), C.byref(self._p), self._acc, None,
                                              self._stream))
        self._next += int(spp)
        return self.samples

    def sums(self) -> np.ndarray:
        """The raw integer sums, uint64 (rows, width, 3), in 2^-24 units
        (rt_accum_read): what ranks exchange for shard.combine_exact."""
        out = np.empty(self.shape, np.uint64)
        self._check(self._dll.rt_accum_read(self._acc, u64ptr(out), self._stream))
        return out

    def add_sums(self, sums, samples: int) -> int:
        """Add another accumulator's sums() and its sample count (rt_accum_add)."""
        sums = np.ascontiguousarray(sums, np.uint64)
        if sums.shape != self.shape:
            raise ValueError(f"Progressive.add_sums: sums must be uint64 {self.shape}")
        self._check(self._dll.rt_accum_add(self._acc, u64ptr(sums), int(samples), self._stream))
        return self.samples

    def frame(self) -> np.ndarray:
        """The frame so far, float32 (rows, width, 3): the sums copied back
        and converted by rt_resolve_sums, whose bits are rt_accum_resolve's."""
        s = self.sums()
        out = np.empty(self.shape, np.float32)
        self._check(self._dll.rt_resolve_sums(u64ptr(s), s.size, self.samples, self._p.flags, fptr(out)))
        return out

    def frame_u8(self) -> np.ndarray:
        """write-color!'s bytes of frame() (the bytes rt_accum_resolve_u8 gives)."""
        return write_color(self.frame())

    def resolve_into(self, d_out: int, u8: bool = False) -> None:
        """Enqueue the conversion into a device buffer the caller owns (its
        address; float32 or, with u8, bytes of `shape`): rt_accum_resolve /
        rt_accum_resolve_u8 on the stream, no copy back."""
        fn = self._dll.rt_accum_resolve_u8 if u8 else self._dll.rt_accum_resolve
        self._check(fn(self._acc, self._p.flags, C.c_void_p(d_out), self._stream))

    def clear(self) -> None:
        """Back to no samples (rt_accum_clear); the next add() starts at the
        first sample index again."""
        self._check(self._dll.rt_accum_clear(self._acc, self._stream))
        self._next = self._first

    def restart(self, cam: rt_camera, sample_begin: int) -> None:
        """Another frame in the same accumulator (a sequence's next frame):
        clear(), then the passes are `cam`'s, from sample index `sample_begin`."""
        self.cam = cam
        self._first = int(sample_begin)
        self.clear()

    def close(self) -> None:
        if getattr(self, "_acc", None):
            self._dll.rt_accum_free(self._acc)
            self._acc = C.c_void_p()
        if getattr(self, "_ds", None):
            self._dll.rt_scene_free(self._ds)
            self._ds = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


class Adaptive:
    """compute-pixel's sample loop (raytracing.clj:141-155) run only where it
    still changes the picture (rt_adapt, include/rt.h): the samples go into
    two half accumulators by turns, and an 8 x 8 tile whose halves agree
    within tol_q16 / 65536 (relative L1) after at least min_spp samples, or
    which reaches max_spp, is traced no more.  Every tile of frame() is bit
    for bit that tile of one launch at spp = counts()[tile].

        ad = Adaptive(scene, cam, 400, 225, tol_q16=2048, step=10, min_spp=20, max_spp=100)
        ad.run(); show(ad.frame_u8()); heat = ad.counts()

    `stream`: a HIP stream handle (int) for the steps and copies, default the
    NULL stream."""

    def __init__(self, scene, cam: rt_camera, width: int, height: int, tol_q16: int = 2048, step: int = 8,
                 min_spp: int = 16, max_spp: int = 64, max_depth: int = 50, seed: int = 1, rows=None,
                 row_tile: int = 8, tile_first: int = 0, tile_step: int = 0, flags: int = 0, sample_begin: int = 0,
                 device: int = 0, stream=None, library=None):
        self._dll = library if library is not None else lib
        self.scene = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
        self.cam = cam
        r0, r1 = (0, height) if rows is None else rows
        self._p = rt_params(width=width, height=height, row_begin=r0, row_end=r1, spp=0, max_depth=max_depth,
                            seed=seed, sample_begin=sample_begin, row_tile=row_tile, tile_first=tile_first,
                            tile_step=tile_step, flags=flags)
        self.opts = rt_adapt_opts(step_spp=int(step), min_spp=int(min_spp), max_spp=int(max_spp), tol_q16=int(tol_q16))
        self._stream = C.c_void_p(stream) if stream else None
        self._ds, self._ad = C.c_void_p(), C.c_void_p()
        self._check(self._dll.rt_scene_upload(int(device), C.byref(self.scene.c), C.byref(self._ds)))
        try:
            self._check(self._dll.rt_adapt_create(self._ds, C.byref(self._p), C.byref(self.opts), C.byref(self._ad)))
        except RTError:
            self.close()
            raise
        self.shape = (self._dll.rt_rows_out(C.byref(self._p)), width, 3)
        self.tiles = ((self.shape[0] + 7) // 8, (width + 7) // 8)

    def _check(self, code):
        if code < 0:
            raise RTError(code, self._dll.rt_last_error().decode(errors="replace"))
        return code

    @property
    def samples_traced(self) -> int:
        """Samples traced so far, summed over pixels (rt_adapt_samples)."""
        return int(self._dll.rt_adapt_samples(self._ad))

    @property
    def active(self) -> int:
        """Tiles still active as of the last test read back (rt_adapt_active)."""
        return int(self._dll.rt_adapt_active(self._ad))

    def step(self) -> int:
        """Enqueue one step (rt_adapt_step); returns the tiles it traces, 0
        once every tile has stopped."""
        return self._check(self._dll.rt_adapt_step(self._ds, C.byref(self.cam), C.byref(self._p), self._ad, None,
                                                   self._stream))

    def run(self) -> int:
        """Steps until no tile is active; returns their number."""
        n = 0
        while self.step() > 0:
            n += 1
        return n

    def counts(self) -> np.ndarray:
        """Samples per pixel of each 8 x 8 tile, uint32 (gy, gx): the heat map."""
        out = np.empty(self.tiles, np.uint32)
        self._check(self._dll.rt_adapt_counts(self._ad, u32ptr(out), self._stream))
        return out

    def halves(self):
        """The two halves' integer sums, uint64 (rows, width, 3) each (rt_adapt_read)."""
        h0, h1 = np.empty(self.shape, np.uint64), np.empty(self.shape, np.uint64)
        self._check(self._dll.rt_adapt_read(self._ad, u64ptr(h0), u64ptr(h1), self._stream))
        return h0, h1

    def frame(self) -> np.ndarray:
        """The frame so far, float32 (rows, width, 3): the halves and counts
        copied back and converted by rt_adapt_resolve_host, whose bits are
        rt_adapt_resolve's."""
        h0, h1 = self.halves()
        counts = self.counts()
        out = np.empty(self.shape, np.float32)
        self._check(self._dll.rt_adapt_resolve_host(u64ptr(h0), u64ptr(h1), u32ptr(counts), self.shape[1],
                                                    self.shape[0], self._p.flags, fptr(out)))
        return out

    def frame_u8(self) -> np.ndarray:
        """write-color!'s bytes of frame() (the bytes rt_adapt_resolve_u8 gives)."""
        return write_color(self.frame())

    def resolve_into(self, d_out: int, u8: bool = False) -> None:
        """Enqueue the conversion into a device buffer the caller owns
        (rt_adapt_resolve / rt_adapt_resolve_u8 on the stream, no copy back)."""
        fn = self._dll.rt_adapt_resolve_u8 if u8 else self._dll.rt_adapt_resolve
        self._check(fn(self._ad, self._p.flags, C.c_void_p(d_out), self._stream))

    def resolve_half_into(self, d_out: int, half: int) -> None:
        """Enqueue one half (0 or 1) as a frame of its own into a device
        buffer the caller owns (rt_adapt_resolve_half): the two estimates
        Denoiser.run takes, with no trip through the host."""
        self._check(self._dll.rt_adapt_resolve_half(self._ad, int(half), self._p.flags, C.c_void_p(d_out),
                                                    self._stream))

    def clear(self) -> None:
        """Back to step 0 with every tile active (rt_adapt_clear)."""
        self._check(self._dll.rt_adapt_clear(self._ad, self._stream))

    def close(self) -> None:
        if getattr(self, "_ad", None):
            self._dll.rt_adapt_free(self._ad)
            self._ad = C.c_void_p()
        if getattr(self, "_ds", None):
            self._dll.rt_scene_free(self._ds)
            self._ds = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def _chain_opts(chain):
    """`chain` as the hosts take it -> rt_feat_chain_opts, or None for a
    first-hit pass: None or False, True (the defaults), an int (max_bounces),
    or a dict of max_bounces, fuzz_max."""
    if chain is None or chain is False:
        return None
    if chain is True:
        chain = {}
    elif isinstance(chain, (int, np.integer)):
        chain = dict(max_bounces=int(chain))
    unknown = set(chain) - set(CHAIN_DEFAULTS)
    if unknown:
        raise TypeError(f"chain: unknown option(s) {sorted(unknown)}")
    o = {**CHAIN_DEFAULTS, **chain}
    return rt_feat_chain_opts(max_bounces=int(o["max_bounces"]), fuzz_max=float(o["fuzz_max"]))


def feat_chain_host(scene, rays, library=None, **opts) -> np.ndarray:
    """rt_feat_chain_host (include/rt.h): the specular chain of each ray on the
    host, in plain C++ -- per sample what a Features(chain=...) pass adds on the
    device.  rays: float32 (..., 6), origin and un-normalised direction.
    Options: max_bounces, fuzz_max.  Returns a record array of rays' leading
    shape with fields body (-1: the sky), bounces, length (+inf on the sky),
    albedo (3,), normal (3,)."""
    dll = library if library is not None else lib
    sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
    o = _chain_opts(dict(opts))
    rays = np.ascontiguousarray(rays, np.float32)
    if rays.ndim < 1 or rays.shape[-1] != 6:
        raise ValueError("feat_chain_host: rays must be (..., 6)")
    out = np.zeros(rays.shape[:-1], np.dtype(CHAIN_SAMPLE_DTYPE))
    assert out.dtype.itemsize == C.sizeof(rt_chain_sample)
    code = dll.rt_feat_chain_host(C.byref(sc.c), C.byref(o), fptr(rays), out.size,
                                  out.ctypes.data_as(C.POINTER(rt_chain_sample)))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out


class Features:
    """First-hit feature buffers (rt_feat, include/rt.h): per pixel the albedo,
    normal, depth and coverage of the first surface the pixel's camera rays
    meet -- the very rays render() / Progressive trace for the same seed and
    sample indices -- accumulated pass by pass as exact integer sums.

        ft = Features(scene, cam, 400, 225, seed=1)
        ft.add(16)
        f = ft.frame()          # (rows, width, 8): albedo rgb, normal xyz, depth, coverage

    Two choices to know: depth is the NEAREST hit of the pixel's samples (+inf
    where none hit), not a mean; the normal is the mean over all samples with
    misses as zero, not re-normalised.  add() advances sample_begin itself;
    frame() and raw() wait for the passes enqueued on `stream`.

    With `chain` (True, an int max_bounces, or a dict of max_bounces, fuzz_max:
    rt_feat_chain_opts) every pass is a specular-chain pass
    (rt_launch_feat_chain): the features of what mirrors and glass show.  Its
    depth is the path length along the bends: guides for Denoiser.run and
    upsample_into, never for Temporal.step or Temporal.probe."""

    def __init__(self, scene, cam: rt_camera, width: int, height: int, seed: int = 1, flags: int = 0, rows=None,
                 row_tile: int = 8, tile_first: int = 0, tile_step: int = 0, sample_begin: int = 0,
                 device: int = 0, stream=None, library=None, chain=None):
        self._dll = library if library is not None else lib
        self._chain = _chain_opts(chain)
        self.scene = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
        self.cam = cam
        r0, r1 = (0, height) if rows is None else rows
        self._p = rt_params(width=width, height=height, row_begin=r0, row_end=r1, spp=0, max_depth=1, seed=seed,
                            sample_begin=sample_begin, row_tile=row_tile, tile_first=tile_first,
                            tile_step=tile_step, flags=flags)
        self._first, self._next = sample_begin, sample_begin
        self._stream = C.c_void_p(stream) if stream else None
        self._ds, self._ft = C.c_void_p(), C.c_void_p()
        self._check(self._dll.rt_scene_upload(int(device), C.byref(self.scene.c), C.byref(self._ds)))
        try:
            self._check(self._dll.rt_feat_create(self._ds, C.byref(self._p), C.byref(self._ft)))
        except RTError:
            self.close()
            raise
        self.shape = (self._dll.rt_rows_out(C.byref(self._p)), width, RT_FEAT_CHANNELS)

    def _check(self, code):
        if code < 0:
            raise RTError(code, self._dll.rt_last_error().decode(errors="replace"))
        return code

    @property
    def samples(self) -> int:
        """Samples per pixel added so far (rt_feat_samples)."""
        return int(self._dll.rt_feat_samples(self._ft))

    def add(self, spp: int, d_counters=None) -> int:
        """Enqueue one pass of `spp` more samples per pixel (rt_launch_feat, or
        rt_launch_feat_chain with `chain`); returns the new count.  d_counters:
        the address of two device uint64, += {segments, samples}."""
        if spp < 0:
            raise ValueError("Features.add: spp < 0")
        self._p.spp = int(spp)
        self._p.sample_begin = self._next
        cnt = C.c_void_p(d_counters) if d_counters else None
        if self._chain is None:
            self._check(self._dll.rt_launch_feat(self._ds, C.byref(self.cam), C.byref(self._p), self._ft, cnt,
                                                 self._stream))
        else:
            self._check(self._dll.rt_launch_feat_chain(self._ds, C.byref(self.cam), C.byref(self._p),
                                                       C.byref(self._chain), self._ft, cnt, self._stream))
        self._next += int(spp)
        return self.samples

    def raw(self):
        """(sums int64 (rows, width, 6), hits uint32 (rows, width), depth
        float32 (rows, width)): the integer sums in 2^-24 units (albedo rgb,
        normal xyz), the hit counts and the nearest distances (rt_feat_read)."""
        rows, width, _ = self.shape
        sums = np.empty((rows, width, 6), np.int64)
        hits = np.empty((rows, width), np.uint32)
        depth = np.empty((rows, width), np.float32)
        self._check(self._dll.rt_feat_read(self._ft, i64ptr(sums), u32ptr(hits), fptr(depth), self._stream))
        return sums, hits, depth

    def add_raw(self, sums, hits, depth, samples: int) -> int:
        """Merge another Features' raw() and its sample count (rt_feat_add):
        sums and hits added, depth by minimum."""
        rows, width, _ = self.shape
        sums = np.ascontiguousarray(sums, np.int64)
        hits = np.ascontiguousarray(hits, np.uint32)
        depth = np.ascontiguousarray(depth, np.float32)
        if sums.shape != (rows, width, 6) or hits.shape != (rows, width) or depth.shape != (rows, width):
            raise ValueError(f"Features.add_raw: arrays must be ({rows}, {width}[, 6])")
        self._check(self._dll.rt_feat_add(self._ft, i64ptr(sums), u32ptr(hits), fptr(depth), int(samples),
                                          self._stream))
        return self.samples

    def frame(self) -> np.ndarray:
        """The features so far, float32 (rows, width, 8): raw() converted by
        rt_feat_resolve_host, whose bits are rt_feat_resolve's."""
        sums, hits, depth = self.raw()
        out = np.empty(self.shape, np.float32)
        self._check(self._dll.rt_feat_resolve_host(i64ptr(sums), u32ptr(hits), fptr(depth), hits.size, self.samples,
                                                   fptr(out)))
        return out

    def resolve_into(self, d_out: int) -> None:
        """Enqueue the conversion into a device buffer the caller owns (its
        address; float32 of `shape`): rt_feat_resolve on the stream."""
        self._check(self._dll.rt_feat_resolve(self._ft, C.c_void_p(d_out), self._stream))

    def clear(self) -> None:
        """Back to no samples (rt_feat_clear); the next add() starts at the
        first sample index again."""
        self._check(self._dll.rt_feat_clear(self._ft, self._stream))
        self._next = self._first

    def restart(self, cam: rt_camera, sample_begin: int) -> None:
        """Another frame in the same buffers (a sequence's next frame):
        clear(), then the passes are `cam`'s, from sample index `sample_begin`."""
        self.cam = cam
        self._first = int(sample_begin)
        self.clear()

    def close(self) -> None:
        if getattr(self, "_ft", None):
            self._dll.rt_feat_free(self._ft)
            self._ft = C.c_void_p()
        if getattr(self, "_ds", None):
            self._dll.rt_scene_free(self._ds)
            self._ds = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def _denoise_opts(opts: dict) -> rt_denoise_opts:
    unknown = set(opts) - set(DENOISE_DEFAULTS)
    if unknown:
        raise TypeError(f"denoise: unknown option(s) {sorted(unknown)}")
    o = {**DENOISE_DEFAULTS, **opts}
    return rt_denoise_opts(levels=int(o["levels"]), normal_pow2=int(o["normal_pow2"]), sigma_c=float(o["sigma_c"]),
                           sigma_z=float(o["sigma_z"]))


def denoise_host(half0, half1, feat, library=None, **opts) -> np.ndarray:
    """rt_denoise_host (include/rt.h): the feature-guided a-trous filter on the
    host, in plain C++ -- the bits Denoiser.run gives on the device.  half0,
    half1: float32 (rows, width, 3), two estimates of the frame from disjoint,
    equally large sample sets; feat: float32 (rows, width, 8) as Features.frame()
    gives it.  Options: levels, normal_pow2, sigma_c, sigma_z.  Returns float32
    (rows, width, 3)."""
    dll = library if library is not None else lib
    half0 = np.ascontiguousarray(half0, np.float32)
    half1 = np.ascontiguousarray(half1, np.float32)
    feat = np.ascontiguousarray(feat, np.float32)
    if half0.ndim != 3 or half0.shape[2] != 3 or half1.shape != half0.shape or \
            feat.shape != half0.shape[:2] + (RT_FEAT_CHANNELS,):
        raise ValueError("denoise_host: half0, half1 must be (rows, width, 3) and feat (rows, width, 8)")
    rows, width = half0.shape[:2]
    out = np.empty(half0.shape, np.float32)
    o = _denoise_opts(opts)
    code = dll.rt_denoise_host(C.byref(o), fptr(half0), fptr(half1), fptr(feat), width, rows, fptr(out))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out


class Denoiser:
    """The feature-guided a-trous filter on device `device` for images of
    rows x width (rt_denoiser, include/rt.h): it owns the filter's scratch.

        with Denoiser(400, 225) as dn:
            dn.run(d_half0, d_half1, d_feat, d_out)      # device addresses

    run() is asynchronous, on `stream` (a HIP stream handle, int; default the
    NULL stream); the inputs are two half-frames (rows, width, 3) and the
    resolved features (rows, width, 8), all float32 on the device."""

    def __init__(self, width: int, rows: int, device: int = 0, library=None):
        self._dll = library if library is not None else lib
        self.width, self.rows = int(width), int(rows)
        self._dn = C.c_void_p()
        self._check(self._dll.rt_denoiser_create(int(device), self.width, self.rows, C.byref(self._dn)))
        self.shape = (self.rows, self.width, 3)

    def _check(self, code):
        if code < 0:
            raise RTError(code, self._dll.rt_last_error().decode(errors="replace"))
        return code

    def run(self, d_half0: int, d_half1: int, d_feat: int, d_out: int, stream=None, **opts) -> None:
        """Enqueue the filter (rt_denoise); options as denoise_host."""
        o = _denoise_opts(opts)
        self._check(self._dll.rt_denoise(self._dn, C.byref(o), C.c_void_p(d_half0), C.c_void_p(d_half1),
                                         C.c_void_p(d_feat), C.c_void_p(d_out),
                                         C.c_void_p(stream) if stream else None))

    def close(self) -> None:
        if getattr(self, "_dn", None):
            self._dll.rt_denoiser_free(self._dn)
            self._dn = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def render_denoised(scene, cam: rt_camera, width: int, height: int, spp: int = 8, max_depth: int = 50, seed: int = 1,
                    flags: int = 0, library=None, chain=None, **opts):
    """A low-sample frame and its denoised version, on device 0: two
    accumulators of spp / 2 samples each (sample indices [0, spp / 2) and
    [spp / 2, spp): together the rays render() traces at spp), the first-hit
    features of all spp samples, everything resolved on the device, then
    Denoiser.run.  `spp` must be even.  Returns (denoised, mean, feat):
    float32 (height, width, 3), the plain mean of the two halves likewise, and
    the feature frame (height, width, 8).  The device buffers are torch's
    (import torch before rtclj, as the GPU tests and bench.py do: both bring
    a HIP runtime and the first one loaded serves the process).  With `chain`
    (as Features takes it) the guides are specular-chain features: what a
    mirror or glass shows is filtered along its own edges."""
    if spp <= 0 or spp % 2:
        raise ValueError("render_denoised: spp must be even and positive")
    _chain_opts(chain)
    import torch
    if not torch.cuda.is_available():
        raise RTError(-5, "render_denoised: torch sees no GPU (import torch before rtclj)")
    half = spp // 2
    sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
    dev = torch.device("cuda", 0)
    n_px = width * height
    d_h = [torch.empty(n_px * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    d_feat = torch.empty(n_px * RT_FEAT_CHANNELS, dtype=torch.float32, device=dev)
    d_out = torch.empty(n_px * 3, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)   # (the passes below run on the NULL stream)
    with Progressive(sc, cam, width, height, max_depth, seed, flags=flags, library=library) as a0, \
            Progressive(sc, cam, width, height, max_depth, seed, flags=flags, sample_begin=half, library=library) as a1, \
            Features(sc, cam, width, height, seed=seed, flags=flags, library=library, chain=chain) as ft, \
            Denoiser(width, height, library=library) as dn:
        a0.add(half)
        a1.add(half)
        ft.add(spp)
        a0.resolve_into(d_h[0].data_ptr())
        a1.resolve_into(d_h[1].data_ptr())
        ft.resolve_into(d_feat.data_ptr())
        dn.run(d_h[0].data_ptr(), d_h[1].data_ptr(), d_feat.data_ptr(), d_out.data_ptr(), **opts)
        torch.cuda.synchronize(dev)
        h0, h1 = (d.cpu().numpy().reshape(height, width, 3) for d in d_h)
        feat = d_feat.cpu().numpy().reshape(height, width, RT_FEAT_CHANNELS)
        out = d_out.cpu().numpy().reshape(height, width, 3)
    return out, np.float32(0.5) * (h0 + h1), feat


def camera_coarsen(cam: rt_camera, scale: int, library=None) -> rt_camera:
    """rt_camera_coarsen (include/rt.h): the camera of the frame of
    ceil(width / scale) x ceil(height / scale) pixels whose pixel covers a
    scale x scale block of `cam`'s pixels (raytracing.clj:129-135)."""
    dll = library if library is not None else lib
    out = rt_camera()
    code = dll.rt_camera_coarsen(C.byref(cam), int(scale), C.byref(out))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out


def coarse_size(width: int, height: int, scale: int):
    """(ceil(width / scale), ceil(height / scale)): the frame camera_coarsen's camera draws."""
    return -(-int(width) // int(scale)), -(-int(height) // int(scale))


def _upsample_opts(opts: dict) -> rt_upsample_opts:
    unknown = set(opts) - set(UPSAMPLE_DEFAULTS)
    if unknown:
        raise TypeError(f"upsample: unknown option(s) {sorted(unknown)}")
    o = {**UPSAMPLE_DEFAULTS, **opts}
    return rt_upsample_opts(scale=int(o["scale"]), normal_pow2=int(o["normal_pow2"]), sigma_z=float(o["sigma_z"]))


def upsample_host(half0, half1, feat_coarse, feat, library=None, **opts):
    """rt_upsample_host (include/rt.h): guided upsampling on the host, in plain
    C++ -- the bits upsample_into gives on the device.  half0, half1: float32
    (ceil(rows / scale), ceil(width / scale), 3), the coarse frame's two
    estimates (half1 may be None: one image); feat_coarse: float32 of the same
    extent with 8 channels; feat: float32 (rows, width, 8), the full-size
    features.  Options: scale, normal_pow2, sigma_z.  Returns (out0, out1),
    float32 (rows, width, 3) each -- out0 alone when half1 is None."""
    dll = library if library is not None else lib
    o = _upsample_opts(opts)
    half0 = np.ascontiguousarray(half0, np.float32)
    half1 = None if half1 is None else np.ascontiguousarray(half1, np.float32)
    feat_coarse = np.ascontiguousarray(feat_coarse, np.float32)
    feat = np.ascontiguousarray(feat, np.float32)
    if feat.ndim != 3 or feat.shape[2] != RT_FEAT_CHANNELS:
        raise ValueError("upsample_host: feat must be (rows, width, 8)")
    rows, width = feat.shape[:2]
    cshape = (-(-rows // max(o.scale, 1)), -(-width // max(o.scale, 1)))
    if half0.shape != cshape + (3,) or (half1 is not None and half1.shape != half0.shape) or \
            feat_coarse.shape != cshape + (RT_FEAT_CHANNELS,):
        raise ValueError(f"upsample_host: half0, half1 must be {cshape + (3,)} and feat_coarse {cshape + (8,)}")
    out0 = np.empty((rows, width, 3), np.float32)
    out1 = None if half1 is None else np.empty((rows, width, 3), np.float32)
    code = dll.rt_upsample_host(C.byref(o), fptr(half0), None if half1 is None else fptr(half1), fptr(feat_coarse),
                                fptr(feat), width, rows, fptr(out0), None if out1 is None else fptr(out1))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out0 if out1 is None else (out0, out1)


def upsample_into(d_half0: int, d_half1, d_feat_coarse: int, d_feat: int, width: int, rows: int, d_out0: int, d_out1,
                  stream=None, library=None, **opts) -> None:
    """Enqueue rt_upsample on device addresses (float32 buffers the caller
    owns, shaped as upsample_host's; d_half1 and d_out1 both None: one image),
    on `stream` (a HIP stream handle, int; default the NULL stream) of the
    device that holds d_out0.  `width`, `rows`: the full size."""
    dll = library if library is not None else lib
    o = _upsample_opts(opts)
    code = dll.rt_upsample(C.byref(o), C.c_void_p(d_half0), C.c_void_p(d_half1) if d_half1 else None,
                           C.c_void_p(d_feat_coarse), C.c_void_p(d_feat), int(width), int(rows), C.c_void_p(d_out0),
                           C.c_void_p(d_out1) if d_out1 else None, C.c_void_p(stream) if stream else None)
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))


def render_upscaled(scene, cam: rt_camera, width: int, height: int, spp: int = 8, scale: int = 2, max_depth: int = 50,
                    seed: int = 1, flags: int = 0, library=None, upsample=None, stages: bool = False, chain=None,
                    **opts):
    """render_denoised with the colour traced at a render scale, on device 0:
    the two accumulators (spp / 2 samples per coarse pixel each) and a second
    Features (spp samples) run on camera_coarsen(cam, scale) at the coarse
    size; the full-size Features of `cam` (spp samples) guide upsample_into,
    whose two outputs feed Denoiser.run at full size.  `spp` must be even;
    `upsample`: a dict of normal_pow2, sigma_z (rt_upsample_opts); further
    keywords are the denoiser's.  Returns (denoised, mean, feat) as
    render_denoised does -- mean of the two upsampled halves; with `stages`
    (denoised, up0, up1, feat, half0, half1, feat_coarse).  With `chain` (as
    Features takes it) both the coarse and the full-size features are
    specular-chain features: a reflection comes back along its own edges."""
    if spp <= 0 or spp % 2:
        raise ValueError("render_upscaled: spp must be even and positive")
    _chain_opts(chain)
    uopts = dict(upsample or {}, scale=scale)
    _upsample_opts(uopts)
    _denoise_opts(opts)
    import torch
    if not torch.cuda.is_available():
        raise RTError(-5, "render_upscaled: torch sees no GPU (import torch before rtclj)")
    half = spp // 2
    sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
    ccam = camera_coarsen(cam, scale, library=library)
    cw, ch = coarse_size(width, height, scale)
    dev = torch.device("cuda", 0)
    n_px, n_c = width * height, cw * ch
    d_h = [torch.empty(n_c * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    d_fc = torch.empty(n_c * RT_FEAT_CHANNELS, dtype=torch.float32, device=dev)
    d_up = [torch.empty(n_px * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    d_feat = torch.empty(n_px * RT_FEAT_CHANNELS, dtype=torch.float32, device=dev)
    d_out = torch.empty(n_px * 3, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)   # (the passes below run on the NULL stream)
    with Progressive(sc, ccam, cw, ch, max_depth, seed, flags=flags, library=library) as a0, \
            Progressive(sc, ccam, cw, ch, max_depth, seed, flags=flags, sample_begin=half, library=library) as a1, \
            Features(sc, ccam, cw, ch, seed=seed, flags=flags, library=library, chain=chain) as fc, \
            Features(sc, cam, width, height, seed=seed, flags=flags, library=library, chain=chain) as ft, \
            Denoiser(width, height, library=library) as dn:
        a0.add(half)
        a1.add(half)
        fc.add(spp)
        ft.add(spp)
        a0.resolve_into(d_h[0].data_ptr())
        a1.resolve_into(d_h[1].data_ptr())
        fc.resolve_into(d_fc.data_ptr())
        ft.resolve_into(d_feat.data_ptr())
        upsample_into(d_h[0].data_ptr(), d_h[1].data_ptr(), d_fc.data_ptr(), d_feat.data_ptr(), width, height,
                      d_up[0].data_ptr(), d_up[1].data_ptr(), library=library, **uopts)
        dn.run(d_up[0].data_ptr(), d_up[1].data_ptr(), d_feat.data_ptr(), d_out.data_ptr(), **opts)
        torch.cuda.synchronize(dev)
        u0, u1 = (d.cpu().numpy().reshape(height, width, 3) for d in d_up)
        feat = d_feat.cpu().numpy().reshape(height, width, RT_FEAT_CHANNELS)
        out = d_out.cpu().numpy().reshape(height, width, 3)
        if stages:
            h0, h1 = (d.cpu().numpy().reshape(ch, cw, 3) for d in d_h)
            return out, u0, u1, feat, h0, h1, d_fc.cpu().numpy().reshape(ch, cw, RT_FEAT_CHANNELS)
    return out, np.float32(0.5) * (u0 + u1), feat


def _temporal_opts(opts: dict) -> rt_temporal_opts:
    unknown = set(opts) - set(TEMPORAL_DEFAULTS)
    if unknown:
        raise TypeError(f"temporal: unknown option(s) {sorted(unknown)}")
    o = {**TEMPORAL_DEFAULTS, **opts}
    return rt_temporal_opts(max_history=int(o["max_history"]), sigma_z=float(o["sigma_z"]),
                            normal_min=float(o["normal_min"]))


def _temporal_clamp_opts(clamp: dict) -> rt_temporal_clamp_opts:
    unknown = set(clamp) - set(TEMPORAL_CLAMP_DEFAULTS)
    if unknown:
        raise TypeError(f"temporal clamp: unknown option(s) {sorted(unknown)}")
    k = {**TEMPORAL_CLAMP_DEFAULTS, **clamp}
    return rt_temporal_clamp_opts(radius=int(k["radius"]), gamma=float(k["gamma"]))


def temporal_host(cam: rt_camera, prev_cam, half0, half1, feat, prev=None, row0: int = 0, library=None, ids=None,
                  motion=None, clamp=None, mult=None, **opts):
    """rt_temporal_host (include/rt.h): one step of temporal accumulation on the
    host, in plain C++ -- the bits Temporal.step gives on the device.  half0,
    half1: float32 (rows, width, 3); feat: float32 (rows, width, 8); cam: the
    camera that drew them.  prev_cam and prev = (a0, a1, guide, length) are
    the previous camera and the history as Temporal.read() gives it -- (rows,
    width, 3) twice, (rows, width, 4), (rows, width) -- or both None: no
    history.  Options: max_history, sigma_z, normal_min.  With `ids` (int32
    (rows, width), as ids_host gives them) it is rt_temporal_host_motion:
    `motion` (float32 (n_bodies, 4), as body_motion gives it; None: no body
    moved) is subtracted for the pixel's body.  With `clamp` (a dict of radius
    and gamma; {}: the defaults) it is rt_temporal_host_clamp: the fetched
    history is held to the current frame's colour box, with or without ids.
    With `mult` (uint32 (ceil(rows / 8), ceil(width / 8)): the sample multiplier
    of every 8 x 8 tile, as budget_plan_host gives them) it is
    rt_temporal_host_budget: the clamped step (clamp None: the defaults) whose
    blend weights the halves as `mult` frames' worth of samples.
    Returns (out0, out1, length):
    the new history's halves and its length; its guides are feat[..., 3:7]."""
    dll = library if library is not None else lib
    half0 = np.ascontiguousarray(half0, np.float32)
    half1 = np.ascontiguousarray(half1, np.float32)
    feat = np.ascontiguousarray(feat, np.float32)
    if half0.ndim != 3 or half0.shape[2] != 3 or half1.shape != half0.shape or \
            feat.shape != half0.shape[:2] + (RT_FEAT_CHANNELS,):
        raise ValueError("temporal_host: half0, half1 must be (rows, width, 3) and feat (rows, width, 8)")
    rows, width = half0.shape[:2]
    if (prev_cam is None) != (prev is None):
        raise ValueError("temporal_host: prev_cam and prev come together")
    hist = [None] * 4
    if prev is not None:
        hist = [np.ascontiguousarray(a, np.float32) for a in prev]
        if [a.shape for a in hist] != [(rows, width, 3), (rows, width, 3), (rows, width, 4), (rows, width)]:
            raise ValueError("temporal_host: prev must be (a0, a1, guide, length) of the frame's size")
    out0, out1 = np.empty(half0.shape, np.float32), np.empty(half0.shape, np.float32)
    length = np.empty((rows, width), np.float32)
    o = _temporal_opts(opts)
    head = (C.byref(o), C.byref(cam), C.byref(prev_cam) if prev_cam is not None else None, width, rows, int(row0),
            fptr(half0), fptr(half1), fptr(feat), *(fptr(a) if a is not None else None for a in hist))
    k = None if clamp is None else _temporal_clamp_opts(clamp)
    outs = (fptr(out0), fptr(out1), fptr(length))
    if mult is not None:
        mult = np.ascontiguousarray(mult, np.uint32)
        if mult.shape != ((rows + 7) // 8, (width + 7) // 8):
            raise ValueError("temporal_host: mult must be uint32 (ceil(rows / 8), ceil(width / 8))")
        if ids is None and motion is not None:
            raise ValueError("temporal_host: motion comes with ids")
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int32)
            if ids.shape != (rows, width):
                raise ValueError("temporal_host: ids must be int32 (rows, width)")
            motion = np.zeros((0, 4), np.float32) if motion is None else np.ascontiguousarray(motion, np.float32)
            if motion.ndim != 2 or motion.shape[1] != 4:
                raise ValueError("temporal_host: motion must be float32 (n_bodies, 4)")
        nb = 0 if ids is None else len(motion)
        code = dll.rt_temporal_host_budget(head[0], C.byref(k) if k is not None else None, *head[1:],
                                           i32ptr(ids) if ids is not None else None, fptr(motion) if nb else None, nb,
                                           u32ptr(mult), *outs)
    elif ids is None:
        if motion is not None:
            raise ValueError("temporal_host: motion comes with ids")
        if k is None:
            code = dll.rt_temporal_host(*head, *outs)
        else:
            code = dll.rt_temporal_host_clamp(head[0], C.byref(k), *head[1:], None, None, 0, *outs)
    else:
        ids = np.ascontiguousarray(ids, np.int32)
        if ids.shape != (rows, width):
            raise ValueError("temporal_host: ids must be int32 (rows, width)")
        motion = np.zeros((0, 4), np.float32) if motion is None else np.ascontiguousarray(motion, np.float32)
        if motion.ndim != 2 or motion.shape[1] != 4:
            raise ValueError("temporal_host: motion must be float32 (n_bodies, 4)")
        tail = (i32ptr(ids), fptr(motion) if len(motion) else None, len(motion), *outs)
        if k is None:
            code = dll.rt_temporal_host_motion(*head, *tail)
        else:
            code = dll.rt_temporal_host_clamp(head[0], C.byref(k), *head[1:], *tail)
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out0, out1, length


def temporal_probe_host(cam: rt_camera, prev_cam, feat, prev=None, row0: int = 0, library=None, ids=None, motion=None,
                        **opts) -> np.ndarray:
    """rt_temporal_host_probe (include/rt.h): per pixel, the history length the
    next step on these inputs would accept -- steps 1-5 of temporal_host, no
    colour involved -- as float32 (rows, width); 0 where it would find none,
    and everywhere without a previous camera.  feat, prev_cam, prev = (a0, a1,
    guide, length) (a0 and a1 are not read and may be None), ids, motion and
    the options as temporal_host."""
    dll = library if library is not None else lib
    feat = np.ascontiguousarray(feat, np.float32)
    if feat.ndim != 3 or feat.shape[2] != RT_FEAT_CHANNELS:
        raise ValueError("temporal_probe_host: feat must be (rows, width, 8)")
    rows, width = feat.shape[:2]
    if (prev_cam is None) != (prev is None):
        raise ValueError("temporal_probe_host: prev_cam and prev come together")
    guide = length = None
    if prev is not None:
        guide, length = np.ascontiguousarray(prev[2], np.float32), np.ascontiguousarray(prev[3], np.float32)
        if guide.shape != (rows, width, 4) or length.shape != (rows, width):
            raise ValueError("temporal_probe_host: prev must be (a0, a1, guide, length) of the frame's size")
    if ids is None and motion is not None:
        raise ValueError("temporal_probe_host: motion comes with ids")
    nb = 0
    if ids is not None:
        ids = np.ascontiguousarray(ids, np.int32)
        if ids.shape != (rows, width):
            raise ValueError("temporal_probe_host: ids must be int32 (rows, width)")
        motion = np.zeros((0, 4), np.float32) if motion is None else np.ascontiguousarray(motion, np.float32)
        if motion.ndim != 2 or motion.shape[1] != 4:
            raise ValueError("temporal_probe_host: motion must be float32 (n_bodies, 4)")
        nb = len(motion)
    out = np.empty((rows, width), np.float32)
    o = _temporal_opts(opts)
    code = dll.rt_temporal_host_probe(C.byref(o), C.byref(cam), C.byref(prev_cam) if prev_cam is not None else None,
                                      width, rows, int(row0), fptr(feat), fptr(guide) if guide is not None else None,
                                      fptr(length) if length is not None else None,
                                      i32ptr(ids) if ids is not None else None, fptr(motion) if nb else None, nb,
                                      fptr(out))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out


def _budget_opts(opts: dict) -> rt_budget_opts:
    unknown = set(opts) - set(BUDGET_DEFAULTS) - {"half_spp"}
    if unknown:
        raise TypeError(f"budget: unknown option(s) {sorted(unknown)}")
    if "half_spp" not in opts:
        raise TypeError("budget: half_spp is required")
    b = {**BUDGET_DEFAULTS, **opts}
    return rt_budget_opts(half_spp=int(b["half_spp"]), target=int(b["target"]), max_mult=int(b["max_mult"]),
                          quantile_64=int(b["quantile_64"]))


def budget_plan_host(length, library=None, **opts) -> np.ndarray:
    """rt_budget_plan_host (include/rt.h): the sample multiplier of every 8 x 8
    tile, uint32 (ceil(rows / 8), ceil(width / 8)), from a float32 (rows, width)
    history length image (temporal_probe_host's).  Options: half_spp
    (required), target, max_mult, quantile_64."""
    dll = library if library is not None else lib
    length = np.ascontiguousarray(length, np.float32)
    if length.ndim != 2:
        raise ValueError("budget_plan_host: length must be (rows, width)")
    rows, width = length.shape
    o = _budget_opts(opts)
    mult = np.empty(((rows + 7) // 8, (width + 7) // 8), np.uint32)
    code = dll.rt_budget_plan_host(C.byref(o), fptr(length), width, rows, u32ptr(mult))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return mult


def budget_units_host(tile_list, mult, half: int, max_mult: int, library=None) -> np.ndarray:
    """rt_budget_units_host (include/rt.h): the fused trace's unit table of one
    half, int32 (U, 2) with U = mult.sum(), from the tiles by descending
    multiplier (int32, every tile once: Budget.tile_list's) and the tiles'
    multipliers (uint32, 1 .. max_mult: Budget.mult's).  Row u is (tile, k |
    2 * max_mult << 8): block k = 2 * pass + half of the tile's sample blocks."""
    dll = library if library is not None else lib
    tile_list = np.ascontiguousarray(tile_list, np.int32).reshape(-1)
    mult = np.ascontiguousarray(mult, np.uint32).reshape(-1)
    if tile_list.size != mult.size:
        raise ValueError("budget_units_host: list and mult must have one entry per tile")
    out = np.empty((max(mult.size, 1) * max(min(int(max_mult), 16), 1), 2), np.int32)
    n = dll.rt_budget_units_host(i32ptr(tile_list), u32ptr(mult), int(mult.size), int(max_mult), int(half), i32ptr(out))
    if n < 0:
        raise RTError(n, dll.rt_last_error().decode(errors="replace"))
    return out[:n].copy()


def tile_bodies_host(scene, cam, params, tile: int, library=None):
    """rt_tile_bodies_host (include/rt.h): the bodies variant 22's prologue lists
    for 8 x 8 tile `tile` of the launch (cam, params: an rt_params), as (body
    indices, places 4 * record + slot), int32 each, in record order.  More than
    14 bodies: the kernel makes no list for the tile."""
    dll = library if library is not None else lib
    cap = max(int(scene.c.n), 1)
    bodies, slots = np.empty(cap, np.int32), np.empty(cap, np.int32)
    n = dll.rt_tile_bodies_host(C.byref(scene.c), C.byref(cam), C.byref(params), int(tile), i32ptr(bodies), i32ptr(slots), cap)
    if n < 0:
        raise RTError(n, dll.rt_last_error().decode(errors="replace"))
    return bodies[:n].copy(), slots[:n].copy()


class Budget:
    """A budgeted frame on an uploaded scene's device (rt_budget, include/rt.h):
    two half accumulators traced at a per-tile multiple of half_spp samples.

        bd = Budget(ds, width, height, half_spp=1, max_depth=50)
        tp.probe(cam, d_feat, d_len)              # how much history per pixel
        bd.plan(d_len)                            # -> a multiplier per 8 x 8 tile
        bd.trace(ds, cam, sample_begin)           # the frame's one host sync
        bd.resolve_half_into(d_h0, 0); bd.resolve_half_into(d_h1, 1)
        tp.step(cam, d_h0, d_h1, d_feat, d_o0, d_o1, clamp={}, d_mult=bd.d_mult)

    `ds` is an rt_dscene handle (DeviceScene.handle or rt_scene_upload's);
    the object holds no reference to it.  Successive frames advance
    sample_begin by 2 * max_mult * half_spp."""

    def __init__(self, ds, width: int, height: int, max_depth: int = 50, seed: int = 1, flags: int = 0, rows=None,
                 library=None, **opts):
        self._dll = library if library is not None else lib
        self.opts = _budget_opts(opts)
        self.width, self.height, self.flags = int(width), int(height), int(flags)
        r0, r1 = rows if rows is not None else (0, height)
        self.rows = r1 - r0
        self.tiles = ((self.rows + 7) // 8, (self.width + 7) // 8)
        self._p = rt_params(width=width, height=height, row_begin=r0, row_end=r1, spp=0, max_depth=max_depth, seed=seed,
                            flags=flags)
        self._bd = C.c_void_p()
        self._check(self._dll.rt_budget_create(ds, C.byref(self._p), C.byref(self.opts), C.byref(self._bd)))

    def _check(self, code):
        if code < 0:
            raise RTError(code, self._dll.rt_last_error().decode(errors="replace"))
        return code

    def plan(self, d_len: int, stream=None) -> None:
        """Start a frame from a device history-length image (rt_budget_plan)."""
        self._check(self._dll.rt_budget_plan(self._bd, C.c_void_p(d_len), C.c_void_p(stream) if stream else None))

    def plan_mult(self, d_mult: int, stream=None) -> None:
        """Start a frame from the caller's uint32 multipliers on the device,
        one per tile (rt_budget_plan_mult); clamped to 1 .. max_mult."""
        self._check(self._dll.rt_budget_plan_mult(self._bd, C.c_void_p(d_mult), C.c_void_p(stream) if stream else None))

    def trace(self, ds, cam: rt_camera, sample_begin: int = 0, stream=None, d_counters=None, fused: bool = False) -> int:
        """Trace the plan (rt_budget_trace; with `fused` rt_budget_trace_fused:
        the same sums from two launches over device-built unit tables); returns
        the number of launches."""
        p = rt_params.from_buffer_copy(self._p)
        p.spp, p.sample_begin = self.opts.half_spp, int(sample_begin)
        fn = self._dll.rt_budget_trace_fused if fused else self._dll.rt_budget_trace
        return self._check(fn(ds, C.byref(cam), C.byref(p), self._bd, C.c_void_p(d_counters) if d_counters else None,
                              C.c_void_p(stream) if stream else None))

    def units(self, half: int, stream=None) -> np.ndarray:
        """The unit table of one half that the plan's fused trace built on the
        device, int32 (U, 2) (rt_budget_units_read)."""
        out = np.empty((self.tiles[0] * self.tiles[1] * self.opts.max_mult, 2), np.int32)
        n = self._check(self._dll.rt_budget_units_read(self._bd, int(half), i32ptr(out),
                                                       C.c_void_p(stream) if stream else None))
        return out[:n].copy()

    def tile_list(self, stream=None) -> np.ndarray:
        """The plan's tiles by descending multiplier, int32 (rt_budget_list_read)."""
        out = np.empty(self.tiles[0] * self.tiles[1], np.int32)
        self._check(self._dll.rt_budget_list_read(self._bd, i32ptr(out), C.c_void_p(stream) if stream else None))
        return out

    @property
    def samples(self) -> int:
        """Samples of the current plan over all pixels (rt_budget_samples)."""
        return int(self._dll.rt_budget_samples(self._bd))

    @property
    def d_mult(self) -> int:
        """The device address of the plan's multipliers (rt_budget_device_mult)."""
        out = C.c_void_p()
        self._check(self._dll.rt_budget_device_mult(self._bd, C.byref(out)))
        return int(out.value)

    def mult(self, stream=None) -> np.ndarray:
        """The plan's multipliers, uint32 (gy, gx) (rt_budget_mult_read)."""
        m = np.empty(self.tiles, np.uint32)
        self._check(self._dll.rt_budget_mult_read(self._bd, u32ptr(m), C.c_void_p(stream) if stream else None))
        return m

    def halves(self, stream=None):
        """(sums0, sums1): both halves' integer sums, uint64 (rows, width, 3) each (rt_budget_read)."""
        s0, s1 = (np.empty((self.rows, self.width, 3), np.uint64) for _ in range(2))
        self._check(self._dll.rt_budget_read(self._bd, u64ptr(s0), u64ptr(s1), C.c_void_p(stream) if stream else None))
        return s0, s1

    def resolve_into(self, d_out: int, stream=None) -> None:
        """Enqueue the whole frame's resolve into device floats (rt_budget_resolve)."""
        self._check(self._dll.rt_budget_resolve(self._bd, self.flags, C.c_void_p(d_out),
                                                C.c_void_p(stream) if stream else None))

    def resolve_half_into(self, d_out: int, half: int, stream=None) -> None:
        """Enqueue one half's resolve into device floats (rt_budget_resolve_half)."""
        self._check(self._dll.rt_budget_resolve_half(self._bd, int(half), self.flags, C.c_void_p(d_out),
                                                     C.c_void_p(stream) if stream else None))

    def close(self) -> None:
        if getattr(self, "_bd", None):
            self._dll.rt_budget_free(self._bd)
            self._bd = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


class Temporal:
    """Temporal accumulation on device `device` for images of rows x width
    whose first row is camera row row0 (rt_temporal, include/rt.h): it owns the
    history -- the accumulated halves, the guides and the length per pixel --
    and the previous camera.

        with Temporal(400, 225) as tp:
            for cam in cameras:
                ...                                          # the resolves
                tp.step(cam, d_half0, d_half1, d_feat, d_out0, d_out1)
                dn.run(d_out0, d_out1, d_feat, d_out)

    step() is asynchronous, on `stream` (a HIP stream handle, int; default the
    NULL stream); steps of one object go on one stream.  The sample indices of
    successive frames must differ."""

    def __init__(self, width: int, rows: int, row0: int = 0, device: int = 0, library=None):
        self._dll = library if library is not None else lib
        self.width, self.rows, self.row0 = int(width), int(rows), int(row0)
        self._tp = C.c_void_p()
        self._check(self._dll.rt_temporal_create(int(device), self.width, self.rows, self.row0, C.byref(self._tp)))
        self.shape = (self.rows, self.width, 3)

    def _check(self, code):
        if code < 0:
            raise RTError(code, self._dll.rt_last_error().decode(errors="replace"))
        return code

    @property
    def frames(self) -> int:
        """Steps since the last reset (rt_temporal_frames)."""
        return int(self._dll.rt_temporal_frames(self._tp))

    def step(self, cam: rt_camera, d_half0: int, d_half1: int, d_feat: int, d_out0: int, d_out1: int, stream=None,
             d_ids=None, d_motion=None, n_bodies: int = 0, clamp=None, d_mult=None, **opts) -> None:
        """Enqueue one step (rt_temporal_step) on device addresses; options as
        temporal_host.  With `d_ids` (int32 (rows, width) on the device, as
        body_ids_into writes them) it is rt_temporal_step_motion: `d_motion`
        is body_motion's table on the device (n_bodies x 4 float32, 16-byte
        aligned).  With `clamp` (a dict of radius and gamma; {}: the defaults)
        it is rt_temporal_step_clamp, with or without d_ids.  With `d_mult`
        (uint32, one per 8 x 8 tile, on the device: Budget.d_mult) it is
        rt_temporal_step_budget: the clamped step (clamp None: the defaults)
        weighted by the tiles' sample multipliers.  All kinds of step may
        alternate on one object."""
        o = _temporal_opts(opts)
        st = C.c_void_p(stream) if stream else None
        if d_ids is None and (d_motion is not None or n_bodies):
            raise ValueError("Temporal.step: d_motion and n_bodies come with d_ids")
        if d_mult is not None:
            k = _temporal_clamp_opts(clamp) if clamp is not None else None
            self._check(self._dll.rt_temporal_step_budget(
                self._tp, C.byref(o), C.byref(k) if k is not None else None, C.byref(cam), C.c_void_p(d_half0),
                C.c_void_p(d_half1), C.c_void_p(d_feat), C.c_void_p(d_ids) if d_ids is not None else None,
                C.c_void_p(d_motion) if d_motion else None, int(n_bodies), C.c_void_p(d_mult), C.c_void_p(d_out0),
                C.c_void_p(d_out1), st))
        elif clamp is not None:
            k = _temporal_clamp_opts(clamp)
            self._check(self._dll.rt_temporal_step_clamp(
                self._tp, C.byref(o), C.byref(k), C.byref(cam), C.c_void_p(d_half0), C.c_void_p(d_half1),
                C.c_void_p(d_feat), C.c_void_p(d_ids) if d_ids is not None else None,
                C.c_void_p(d_motion) if d_motion else None, int(n_bodies), C.c_void_p(d_out0), C.c_void_p(d_out1), st))
        elif d_ids is None:
            self._check(self._dll.rt_temporal_step(self._tp, C.byref(o), C.byref(cam), C.c_void_p(d_half0),
                                                   C.c_void_p(d_half1), C.c_void_p(d_feat), C.c_void_p(d_out0),
                                                   C.c_void_p(d_out1), st))
        else:
            self._check(self._dll.rt_temporal_step_motion(
                self._tp, C.byref(o), C.byref(cam), C.c_void_p(d_half0), C.c_void_p(d_half1), C.c_void_p(d_feat),
                C.c_void_p(d_ids), C.c_void_p(d_motion) if d_motion else None, int(n_bodies), C.c_void_p(d_out0),
                C.c_void_p(d_out1), st))

    def probe(self, cam: rt_camera, d_feat: int, d_len: int, stream=None, d_ids=None, d_motion=None, n_bodies: int = 0,
              **opts) -> None:
        """Enqueue rt_temporal_probe: d_len (float32 (rows, width) on the device)
        = the history length the next step on these inputs would accept.
        Arguments as step's; nothing of the object changes."""
        o = _temporal_opts(opts)
        if d_ids is None and (d_motion is not None or n_bodies):
            raise ValueError("Temporal.probe: d_motion and n_bodies come with d_ids")
        self._check(self._dll.rt_temporal_probe(
            self._tp, C.byref(o), C.byref(cam), C.c_void_p(d_feat), C.c_void_p(d_ids) if d_ids is not None else None,
            C.c_void_p(d_motion) if d_motion else None, int(n_bodies), C.c_void_p(d_len),
            C.c_void_p(stream) if stream else None))

    def read(self, stream=None):
        """(a0, a1, guide, length): the current history copied out behind the
        stream's work (rt_temporal_read), as temporal_host's `prev`."""
        a0, a1 = np.empty(self.shape, np.float32), np.empty(self.shape, np.float32)
        guide = np.empty((self.rows, self.width, 4), np.float32)
        length = np.empty((self.rows, self.width), np.float32)
        self._check(self._dll.rt_temporal_read(self._tp, fptr(a0), fptr(a1), fptr(guide), fptr(length),
                                               C.c_void_p(stream) if stream else None))
        return a0, a1, guide, length

    def reset(self, stream=None) -> None:
        """Forget the history and the previous camera (rt_temporal_reset)."""
        self._check(self._dll.rt_temporal_reset(self._tp, C.c_void_p(stream) if stream else None))

    def close(self) -> None:
        if getattr(self, "_tp", None):
            self._dll.rt_temporal_free(self._tp)
            self._tp = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def render_sequence(scene, cameras, width: int, height: int, spp: int = 4, max_depth: int = 50, seed: int = 1,
                    flags: int = 0, library=None, temporal=None, stages: bool = False, clamp=None, **opts):
    """A sequence of low-sample frames of a static scene, one per camera of
    `cameras`, each temporally accumulated and then denoised, on device 0: a
    generator that yields float32 (height, width, 3) per camera.  Per frame f:
    two accumulators of spp / 2 samples each (sample indices f * spp ... so
    that no frame repeats another's samples), the first-hit features of all
    spp, everything resolved on the device, Temporal.step, Denoiser.run on the
    accumulated halves.  `spp` must be even.  `temporal`: options of the step
    (max_history, sigma_z, normal_min); `clamp`: None, or the colour clamp's
    options (radius, gamma; {}: the defaults) for rt_temporal_step_clamp;
    further keywords: the denoiser's.  With
    `stages` it yields (denoised, half0, half1, feat, acc0, acc1) instead: the
    resolves and the step's outputs beside the frame.  The device buffers are
    torch's (import torch before rtclj, as render_denoised)."""
    if spp <= 0 or spp % 2:
        raise ValueError("render_sequence: spp must be even and positive")
    _denoise_opts(opts)
    topts = dict(temporal or {})
    _temporal_opts(topts)
    if clamp is not None:
        _temporal_clamp_opts(clamp)
        topts["clamp"] = dict(clamp)
    import torch
    if not torch.cuda.is_available():
        raise RTError(-5, "render_sequence: torch sees no GPU (import torch before rtclj)")
    half = spp // 2
    sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
    dev = torch.device("cuda", 0)
    n_px = width * height
    d_h = [torch.empty(n_px * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    d_acc = [torch.empty(n_px * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    d_feat = torch.empty(n_px * RT_FEAT_CHANNELS, dtype=torch.float32, device=dev)
    d_out = torch.empty(n_px * 3, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)   # (the passes below run on the NULL stream)
    cameras = iter(cameras)
    try:
        cam = next(cameras)
    except StopIteration:
        return
    with Progressive(sc, cam, width, height, max_depth, seed, flags=flags, library=library) as a0, \
            Progressive(sc, cam, width, height, max_depth, seed, flags=flags, library=library) as a1, \
            Features(sc, cam, width, height, seed=seed, flags=flags, library=library) as ft, \
            Temporal(width, height, library=library) as tp, Denoiser(width, height, library=library) as dn:
        f = 0
        while cam is not None:
            for acc, begin in ((a0, f * spp), (a1, f * spp + half), (ft, f * spp)):
                acc.restart(cam, begin)
            a0.add(half)
            a1.add(half)
            ft.add(spp)
            a0.resolve_into(d_h[0].data_ptr())
            a1.resolve_into(d_h[1].data_ptr())
            ft.resolve_into(d_feat.data_ptr())
            tp.step(cam, d_h[0].data_ptr(), d_h[1].data_ptr(), d_feat.data_ptr(), d_acc[0].data_ptr(),
                    d_acc[1].data_ptr(), **topts)
            dn.run(d_acc[0].data_ptr(), d_acc[1].data_ptr(), d_feat.data_ptr(), d_out.data_ptr(), **opts)
            torch.cuda.synchronize(dev)
            out = d_out.cpu().numpy().reshape(height, width, 3)
            if stages:
                yield (out,) + tuple(d.cpu().numpy().reshape(height, width, 3) for d in d_h) + \
                    (d_feat.cpu().numpy().reshape(height, width, RT_FEAT_CHANNELS),) + \
                    tuple(d.cpu().numpy().reshape(height, width, 3) for d in d_acc)
            else:
                yield out
            cam = next(cameras, None)
            f += 1


def ids_host(scene, cam: rt_camera, width: int, rows: int, row0: int = 0, library=None) -> np.ndarray:
    """rt_ids_host (include/rt.h): per pixel of a rows x width image whose first
    row is camera row row0, the index of the body the pixel centre's pinhole
    ray meets first, or -1 -- on the host, in plain C++; the integers
    body_ids_into gives on the device.  Returns int32 (rows, width)."""
    dll = library if library is not None else lib
    sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
    out = np.empty((max(int(rows), 0), max(int(width), 0)), np.int32)
    code = dll.rt_ids_host(C.byref(sc.c), C.byref(cam), int(width), int(rows), int(row0), i32ptr(out))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out


def pinhole_rays(cam: rt_camera, width: int, rows: int, row0: int = 0) -> np.ndarray:
    """rt_launch_ids' rays as rt_ray records, (rows, width): origin = center,
    d = ((p00 + x * du) + j * dv) - center with j = row0 + y, each operation
    one float32 operation rounded once, t_min = 1e-3, t_max = inf."""
    f = np.float32
    center, p00, du, dv = (np.array(list(v), f) for v in (cam.center, cam.p00, cam.du, cam.dv))
    x = np.arange(int(width), dtype=f)[None, :, None]
    j = (np.arange(int(rows), dtype=np.int64) + int(row0)).astype(f)[:, None, None]
    rays = np.zeros((int(rows), int(width)), np.dtype(RAY_DTYPE))
    rays["o"] = center
    rays["d"] = ((p00 + x * du) + j * dv) - center
    rays["t_min"] = f(1e-3)
    rays["t_max"] = f(np.inf)
    return rays


def _query_args(scene, rays, last):
    sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
    rays = np.ascontiguousarray(rays, np.dtype(RAY_DTYPE))
    if last is not None:
        last = np.ascontiguousarray(last, np.int32)
        if last.shape != rays.shape:
            raise ValueError("ray query: last must have the rays' shape")
    return sc, rays, last


def rays_host(scene, rays, last=None, library=None) -> np.ndarray:
    """rt_rays_host (include/rt.h): the closest hit of each caller-supplied ray
    on the host, in plain C++ -- the records DeviceScene.intersect_into writes
    on the device, bit for bit.  rays: a record array of RAY_DTYPE (o, t_min,
    d, t_max), any shape; last: None, or int32 of the same shape, the body each
    ray leaves (-1: none).  Returns RAY_HIT_DTYPE records of rays' shape: body
    (-1: none), front_face, t, dist, normal, reserved."""
    dll = library if library is not None else lib
    sc, rays, last = _query_args(scene, rays, last)
    out = np.zeros(rays.shape, np.dtype(RAY_HIT_DTYPE))
    assert out.dtype.itemsize == C.sizeof(rt_ray_hit) and rays.dtype.itemsize == C.sizeof(rt_ray)
    code = dll.rt_rays_host(C.byref(sc.c), rays.ctypes.data_as(C.POINTER(rt_ray)),
                            None if last is None else i32ptr(last), rays.size,
                            out.ctypes.data_as(C.POINTER(rt_ray_hit)))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out


def occluded_host(scene, rays, last=None, library=None) -> np.ndarray:
    """rt_occluded_host (include/rt.h): per ray whether any body is met in
    (t_min, t_max) -- rays_host(...)["body"] >= 0, found with the first body
    the test accepts.  Returns bool of rays' shape."""
    dll = library if library is not None else lib
    sc, rays, last = _query_args(scene, rays, last)
    out = np.zeros(rays.shape, np.uint8)
    code = dll.rt_occluded_host(C.byref(sc.c), rays.ctypes.data_as(C.POINTER(rt_ray)),
                                None if last is None else i32ptr(last), rays.size, u8ptr(out))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out.astype(bool)


def body_ids_into(scene, cam: rt_camera, width: int, height: int, d_ids: int, rows=None, stream=None, device: int = 0,
                  library=None) -> None:
    """rt_launch_ids (include/rt.h) for a scene on the host: upload it, enqueue
    the body-id pass for camera rows `rows` = (first, end) (default: all
    `height`) into d_ids (a device address: int32, (end - first) x width), wait
    for it and free the scene.  A caller with an uploaded scene calls
    rt_launch_ids itself (render_animation does)."""
    dll = library if library is not None else lib
    sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
    r0, r1 = (0, height) if rows is None else rows
    st = C.c_void_p(stream) if stream else None
    ds = C.c_void_p()

    def ok(code):
        if code < 0:
            raise RTError(code, dll.rt_last_error().decode(errors="replace"))

    try:
        ok(dll.rt_scene_upload(int(device), C.byref(sc.c), C.byref(ds)))
        ok(dll.rt_launch_ids(ds, C.byref(cam), int(width), int(r1 - r0), int(r0), C.c_void_p(d_ids), st))
        _stream_wait(st)
    finally:
        dll.rt_scene_free(ds)


def _stream_wait(st) -> None:
    """Wait for a HIP stream's work through torch's runtime (the process's one)."""
    import torch
    if st is None or not st.value:
        torch.cuda.synchronize()
    else:
        torch.cuda.ExternalStream(st.value).synchronize()


def body_motion(cur_scene, prev_scene, library=None) -> np.ndarray:
    """rt_body_motion (include/rt.h): float32 (n, 4), per body its centre's
    displacement from prev_scene to cur_scene (lane 3 is 0); NaN for a body
    whose radius or material changed -- it has no past."""
    dll = library if library is not None else lib
    cur = cur_scene if isinstance(cur_scene, Scene) else Scene.from_bodies(cur_scene)
    prev = prev_scene if isinstance(prev_scene, Scene) else Scene.from_bodies(prev_scene)
    out = np.empty((len(cur), 4), np.float32)
    code = dll.rt_body_motion(C.byref(cur.c), C.byref(prev.c), fptr(out))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out


def schedule_read(ds, stream=None, arrays: bool = True, library=None):
    """rt_schedule_read (include/rt.h): the adaptive tile order's entry of the
    uploaded scene `ds` (a C.c_void_p) on HIP stream `stream` (an address;
    None: the NULL stream).  Returns (info dict, cost uint32 (n_tiles,), order
    int32 (n_tiles,), units int32 (plan_units, 2)); the arrays are empty where
    the entry holds none, and None with arrays=False (info only).  Waits for
    the stream; changes nothing."""
    dll = library if library is not None else lib
    st = C.c_void_p(stream) if stream else None
    info = rt_schedule_info()

    def ok(code):
        if code < 0:
            raise RTError(code, dll.rt_last_error().decode(errors="replace"))

    ok(dll.rt_schedule_read(ds, st, C.byref(info), None, None, None, 0, 0))
    if not arrays:
        return info.as_dict(), None, None, None
    n = info.n_tiles if info.has_record else 0
    u = max(info.plan_units, 0)
    cost, order, units = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros((u, 2), np.int32)
    ok(dll.rt_schedule_read(ds, st, C.byref(info), u32ptr(cost) if n else None, i32ptr(order) if n else None,
                            i32ptr(units) if u else None, n, u))
    return info.as_dict(), cost, order, units


def schedule_sort(cost, units: int = 0, smax: int = 1, device: int = 0, stream=None, library=None):
    """rt_schedule_sort (include/rt.h): the schedule's sort kernel, and for
    units > 0 its split-plan kernel, on `cost` (uint32, one per tile) as a
    launch runs them.  The order and the units go up filled with -1.  Returns
    (halved cost uint32 (n,), order int32 (n,), units int32 (units, 2))."""
    dll = library if library is not None else lib
    c = np.array(cost, dtype=np.uint32).reshape(-1)
    order = np.full(c.size, -1, np.int32)
    tab = np.full((max(int(units), 0), 2), -1, np.int32)
    code = dll.rt_schedule_sort(int(device), u32ptr(c), c.size, i32ptr(order), int(units), int(smax),
                                i32ptr(tab) if tab.size else None, C.c_void_p(stream) if stream else None)
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return c, order, tab


def _spheres(scene) -> np.ndarray:
    if isinstance(scene, Scene):
        return scene.sphere
    if isinstance(scene, np.ndarray):
        return np.ascontiguousarray(scene, np.float32).reshape(-1, 4)
    return Scene.from_bodies(scene).sphere


def tree_build_host(scene, k: int, library=None):
    """rt_tree_build_host (include/rt.h): tree k (0, 1, 2: leaves of 2, 4, 8
    bodies) of a scene (a Scene, a list of bodies or an (n, 4) array of
    spheres) as rt_scene_upload uploads it, built on the host.  Returns
    (rt_tree_info, uint8 array of info.blob_bytes)."""
    dll = library if library is not None else lib
    sph = _spheres(scene)
    info = rt_tree_info()
    dll.rt_tree_build_host(fptr(sph), len(sph), int(k), None, 0, C.byref(info))   # (the size: RT_E_ARG, info filled)
    blob = np.zeros(max(info.blob_bytes, 0), np.uint8)
    code = dll.rt_tree_build_host(fptr(sph), len(sph), int(k), blob.ctypes.data_as(C.c_void_p), blob.size,
                                  C.byref(info))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return info, blob


def tree_refit_host(info: rt_tree_info, blob: np.ndarray, scene_at_upload, scene_now, library=None):
    """rt_tree_refit_host (include/rt.h): the tree (info, blob) built from
    scene_at_upload, refitted to scene_now's spheres on the host -- the bytes
    rt_scene_update leaves on the device.  Returns a new (info, blob); the
    arguments are not written.  RTError (RT_E_ARG) on a changed radius or a
    centre whose finiteness changed."""
    dll = library if library is not None else lib
    s0, s1 = _spheres(scene_at_upload), _spheres(scene_now)
    if len(s0) != len(s1):
        raise ValueError("tree_refit_host: the scenes' body counts differ")
    out_info = rt_tree_info.from_buffer_copy(info)
    out = np.array(blob, np.uint8, copy=True)
    if out.size != info.blob_bytes:
        raise ValueError("tree_refit_host: blob is not info.blob_bytes long")
    code = dll.rt_tree_refit_host(out.ctypes.data_as(C.c_void_p), C.byref(out_info), fptr(s0), fptr(s1), len(s0))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return out_info, out


def tree_cost(info: rt_tree_info, blob: np.ndarray, library=None) -> float:
    """rt_tree_cost_host (include/rt.h): the sum of the child boxes' surface
    areas; its ratio to the value at the upload tells how far refits have
    loosened a tree."""
    dll = library if library is not None else lib
    blob = np.ascontiguousarray(blob, np.uint8)
    if blob.size != info.blob_bytes:
        raise ValueError("tree_cost: blob is not info.blob_bytes long")
    cost = C.c_double()
    code = dll.rt_tree_cost_host(blob.ctypes.data_as(C.c_void_p), C.byref(info), C.byref(cost))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return cost.value


class DeviceScene:
    """A scene on a device (rt_scene_upload) that follows its bodies:
    update(scene) moves them in place (rt_scene_update: same body count,
    radii, kinds and materials; the trees are refitted on the device, in
    stream order, without waiting), tree(k) reads a tree back.  `handle` is the
    rt_dscene* the launch entries take.  A context manager; free() on exit."""

    def __init__(self, scene=None, device: int = 0, library=None):
        self._dll = library if library is not None else lib
        self.device = int(device)
        self.handle = C.c_void_p()
        self.n = 0
        if scene is not None:
            self.upload(scene)

    def _ok(self, code):
        if code < 0:
            raise RTError(code, self._dll.rt_last_error().decode(errors="replace"))
        return code

    def upload(self, scene):
        """A fresh upload (the trees built on the host) in place of what it holds."""
        sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
        self.free()
        self._ok(self._dll.rt_scene_upload(self.device, C.byref(sc.c), C.byref(self.handle)))
        self.n = len(sc)
        return self

    def update(self, scene, stream=None):
        """rt_scene_update with scene's spheres (a Scene, a list of bodies or an
        (n, 4) array), enqueued on `stream` (a HIP stream address; None: the
        default stream).  The array may be reused at once."""
        if not self.handle:
            raise RuntimeError("DeviceScene.update: nothing uploaded")
        sph = _spheres(scene)
        if len(sph) != self.n:
            raise ValueError("DeviceScene.update: the body count differs from the upload's")
        self._ok(self._dll.rt_scene_update(self.handle, fptr(sph) if self.n else None,
                                           C.c_void_p(stream) if stream else None))
        return self

    def intersect_into(self, d_rays: int, n: int, d_hits: int, d_last=None, stream=None):
        """rt_launch_rays: the closest hits of n rays (device address d_rays,
        rt_ray records) into d_hits (device address, rt_ray_hit records),
        enqueued on `stream` (a HIP stream address; None: the default stream).
        d_last: None or the device address of n int32, the body each ray
        leaves.  Asynchronous."""
        self._ok(self._dll.rt_launch_rays(self.handle, C.c_void_p(d_rays), C.c_void_p(d_last) if d_last else None,
                                          int(n), C.c_void_p(d_hits), C.c_void_p(stream) if stream else None))
        return self

    def occluded_into(self, d_rays: int, n: int, d_occluded: int, d_last=None, stream=None):
        """rt_launch_occluded: per ray one byte, 1 iff a body lies in
        (t_min, t_max), into d_occluded (device address, n bytes); the other
        arguments as intersect_into's.  Asynchronous."""
        self._ok(self._dll.rt_launch_occluded(self.handle, C.c_void_p(d_rays), C.c_void_p(d_last) if d_last else None,
                                              int(n), C.c_void_p(d_occluded),
                                              C.c_void_p(stream) if stream else None))
        return self

    def tree_info(self, k: int) -> rt_tree_info:
        info = rt_tree_info()
        self._ok(self._dll.rt_scene_tree_info(self.handle, int(k), C.byref(info)))
        return info

    def tree(self, k: int, stream=None):
        """(rt_tree_info, uint8 array): tree k as the device holds it behind
        `stream`'s work (rt_scene_tree_read: waits for the stream)."""
        info = self.tree_info(k)
        blob = np.zeros(info.blob_bytes, np.uint8)
        self._ok(self._dll.rt_scene_tree_read(self.handle, int(k), blob.ctypes.data_as(C.c_void_p), blob.size,
                                              C.c_void_p(stream) if stream else None))
        return info, blob

    def free(self):
        if self.handle:
            self._dll.rt_scene_free(self.handle)
        self.handle = C.c_void_p()
        self.n = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.free()
        except Exception:   # (interpreter shutdown: the library may be gone)
            pass


def _same_but_centres(a: Scene, b: Scene) -> bool:
    """Whether rt_scene_update can turn a's upload into b: the radii, kinds and
    materials agree bit for bit (rt_body_motion's test for "the same body")."""
    return (len(a) == len(b) and a.sphere[:, 3].tobytes() == b.sphere[:, 3].tobytes()
            and a.kind.tobytes() == b.kind.tobytes() and a.mat.tobytes() == b.mat.tobytes())


def render_animation(scenes, cameras, width: int, height: int, spp: int = 4, max_depth: int = 50, seed: int = 1,
                     flags: int = 0, library=None, temporal=None, stages: bool = False, refit: bool = False, clamp=None,
                     budget=None, scale=None, upsample=None, chain=None, **opts):
    """render_sequence for bodies that move: one Scene per frame (all with the
    same body count), zipped with `cameras`; a generator that yields float32
    (height, width, 3) per frame, on device 0.  Per frame f: the scene's upload
    (rt_scene_upload builds its trees on the host; with `refit` only frame 0
    is uploaded and every later frame is an rt_scene_update, which refits the
    trees on the device -- a frame whose radii, kinds or materials differ from
    frame 0's, or whose update is refused, is uploaded afresh; the bits are the
    same either way, a refitted tree only costs time as it loosens), two
    accumulators of spp / 2 samples each from sample index f * spp, the
    first-hit features of all spp, the body ids (rt_launch_ids), body_motion
    against the previous frame's scene (frame 0: no displacement), the
    motion-aware step (rt_temporal_step_motion) and Denoiser.run.  `spp` must be
    even; `temporal`, `clamp` (with it the step is rt_temporal_step_clamp with
    the ids) and further keywords as render_sequence.  With `stages` it
    yields (denoised, half0, half1, feat, acc0, acc1, ids).  With identical
    scenes it gives render_sequence's bits.
    With `budget` (a dict of half_spp, target, max_mult, quantile_64: rt_budget_opts;
    and `fused`, default False: trace with rt_budget_trace_fused, the same bits
    from two launches) the samples go where the history is short, and `spp` is
    not read: per frame
    the features (a uniform 2 * half_spp, from sample index f * 2 * max_mult *
    half_spp) and the ids come first, then Temporal.probe, Budget.plan,
    Budget.trace from the same index, the two halves' resolves, the weighted
    step (rt_temporal_step_budget with the ids; without `clamp` with gamma =
    +inf, which clamps nothing) and Denoiser.run.  Frame 0 has no history and is
    traced at min(target, max_mult) everywhere.  `stages` then yields the
    tiles' multipliers, uint32 (ceil(height / 8), ceil(width / 8)), as an
    eighth item.  Without `budget` nothing changes.
    With `scale` (2..4) the colour is traced at a render scale: the two
    accumulators and a second rt_feat (spp samples) use camera_coarsen(cam,
    scale) at the coarse size, and upsample_into (options: `upsample`, a dict of
    normal_pow2, sigma_z) brings the two resolved halves up to full size between
    the resolves and the step; the features, ids, motion, step and denoiser stay
    at full size, and the yielded half0, half1 are the upsampled ones.  `stages`
    then yields three more items: the coarse half0, half1 and features.  `scale`
    with `budget` is refused (the budget's tile lists belong to the traced
    grid).  Without `scale` nothing changes.
    With `chain` (as Features takes it) a second full-size rt_feat holds
    specular-chain passes of the same samples and guides Denoiser.run and, with
    `scale`, upsample_into, whose coarse features are chain passes too.  The
    probe and the step keep the first-hit features: a reprojection needs the
    real surface's depth and normal, so their stages are the bits of a run
    without `chain`.  `stages` then yields the chain features as a last item."""
    copt = _chain_opts(chain)
    if scale is not None and budget is not None:
        raise ValueError("render_animation: scale and budget cannot be combined")
    if scale is not None:
        uopts = dict(upsample or {}, scale=scale)
        _upsample_opts(uopts)
    fused = False
    if budget is not None:
        budget = dict(budget)
        fused = bool(budget.pop("fused", False))   # (Budget.trace's, no rt_budget_opts field)
        bopt = _budget_opts(budget)
        spp = 2 * bopt.half_spp
    if spp <= 0 or spp % 2:
        raise ValueError("render_animation: spp must be even and positive")
    _denoise_opts(opts)
    topts = dict(temporal or {})
    _temporal_opts(topts)
    if clamp is not None:
        _temporal_clamp_opts(clamp)
        topts["clamp"] = dict(clamp)
    import torch
    if not torch.cuda.is_available():
        raise RTError(-5, "render_animation: torch sees no GPU (import torch before rtclj)")
    dll = library if library is not None else lib

    def ok(code):
        if code < 0:
            raise RTError(code, dll.rt_last_error().decode(errors="replace"))

    half = spp // 2
    dev = torch.device("cuda", 0)
    n_px = width * height
    d_h = [torch.empty(n_px * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    d_acc = [torch.empty(n_px * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    d_feat = torch.empty(n_px * RT_FEAT_CHANNELS, dtype=torch.float32, device=dev)
    d_ids = torch.empty(n_px, dtype=torch.int32, device=dev)
    d_out = torch.empty(n_px * 3, dtype=torch.float32, device=dev)
    d_motion = None
    d_len = torch.empty(n_px, dtype=torch.float32, device=dev) if budget is not None else None
    stride = spp if budget is None else 2 * bopt.max_mult * bopt.half_spp   # sample indices per frame
    bd = None
    if budget is not None and clamp is None:
        topts["clamp"] = dict(gamma=float("inf"))
    torch.cuda.synchronize(dev)   # (the passes below run on the NULL stream)
    shape = rt_params(width=width, height=height, row_begin=0, row_end=height, spp=0, max_depth=max_depth, seed=seed,
                      flags=flags)
    ds, acc, ft, fc, fch = C.c_void_p(), [C.c_void_p(), C.c_void_p()], C.c_void_p(), C.c_void_p(), C.c_void_p()
    d_chain = torch.empty(n_px * RT_FEAT_CHANNELS, dtype=torch.float32, device=dev) if copt is not None else None
    d_guide = d_feat if copt is None else d_chain   # what the denoiser and the upsampler are guided by

    def launch_feat(cam_, p_, f_, chained):
        if chained and copt is not None:
            ok(dll.rt_launch_feat_chain(ds, C.byref(cam_), C.byref(p_), C.byref(copt), f_, None, None))
        else:
            ok(dll.rt_launch_feat(ds, C.byref(cam_), C.byref(p_), f_, None, None))
    prev_sc = first_sc = None
    traced, d_tr, d_fc = shape, d_h, None   # what the accumulators trace and resolve into
    if scale is not None:
        cw, ch = coarse_size(width, height, scale)
        traced = rt_params(width=cw, height=ch, row_begin=0, row_end=ch, spp=0, max_depth=max_depth, seed=seed,
                           flags=flags)
        d_tr = [torch.empty(cw * ch * 3, dtype=torch.float32, device=dev) for _ in range(2)]
        d_fc = torch.empty(cw * ch * RT_FEAT_CHANNELS, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
    try:
        with Temporal(width, height, library=library) as tp, Denoiser(width, height, library=library) as dn:
            for f, (scene, cam) in enumerate(zip(scenes, cameras)):
                sc = scene if isinstance(scene, Scene) else Scene.from_bodies(scene)
                if prev_sc is not None and len(sc) != len(prev_sc):
                    raise ValueError("render_animation: every scene must have the same body count")
                if refit and ds and _same_but_centres(first_sc, sc) and \
                        dll.rt_scene_update(ds, fptr(sc.sphere) if len(sc) else None, None) >= 0:
                    pass   # (moved in place, in the NULL stream's order)
                else:
                    if ds:   # (refit: a frame rt_scene_update cannot reach)
                        ok(dll.rt_scene_free(ds))
                        ds = C.c_void_p()
                    ok(dll.rt_scene_upload(0, C.byref(sc.c), C.byref(ds)))
                    first_sc = sc
                if f == 0:
                    if budget is None:
                        for a in acc:
                            ok(dll.rt_accum_create(ds, C.byref(traced), C.byref(a)))
                    else:
                        bd = Budget(ds, width, height, max_depth=max_depth, seed=seed, flags=flags, library=library,
                                    **dict(budget))
                    ok(dll.rt_feat_create(ds, C.byref(shape), C.byref(ft)))
                    if scale is not None:
                        ok(dll.rt_feat_create(ds, C.byref(traced), C.byref(fc)))
                    if copt is not None:
                        ok(dll.rt_feat_create(ds, C.byref(shape), C.byref(fch)))
                    motion = np.zeros((len(sc), 4), np.float32)
                else:
                    if budget is None:
                        for a in acc:
                            ok(dll.rt_accum_clear(a, None))
                    ok(dll.rt_feat_clear(ft, None))
                    if scale is not None:
                        ok(dll.rt_feat_clear(fc, None))
                    if copt is not None:
                        ok(dll.rt_feat_clear(fch, None))
                    motion = body_motion(sc, prev_sc, library=library)
                tcam = cam if scale is None else camera_coarsen(cam, scale, library=library)
                if budget is None:
                    for a, begin, n in ((acc[0], f * spp, half), (acc[1], f * spp + half, half)):
                        p = rt_params.from_buffer_copy(traced)
                        p.spp, p.sample_begin = n, begin
                        ok(dll.rt_launch_accum(ds, C.byref(tcam), C.byref(p), a, None, None))
                if scale is not None:
                    p = rt_params.from_buffer_copy(traced)
                    p.spp, p.sample_begin, p.max_depth = spp, f * stride, 1
                    launch_feat(tcam, p, fc, True)
                p = rt_params.from_buffer_copy(shape)
                p.spp, p.sample_begin, p.max_depth = spp, f * stride, 1
                launch_feat(cam, p, ft, False)
                if copt is not None:
                    launch_feat(cam, p, fch, True)
                ok(dll.rt_launch_ids(ds, C.byref(cam), width, height, 0, C.c_void_p(d_ids.data_ptr()), None))
                if budget is None:
                    ok(dll.rt_accum_resolve(acc[0], flags, C.c_void_p(d_tr[0].data_ptr()), None))
                    ok(dll.rt_accum_resolve(acc[1], flags, C.c_void_p(d_tr[1].data_ptr()), None))
                ok(dll.rt_feat_resolve(ft, C.c_void_p(d_feat.data_ptr()), None))
                if copt is not None:
                    ok(dll.rt_feat_resolve(fch, C.c_void_p(d_chain.data_ptr()), None))
                if scale is not None:
                    ok(dll.rt_feat_resolve(fc, C.c_void_p(d_fc.data_ptr()), None))
                    upsample_into(d_tr[0].data_ptr(), d_tr[1].data_ptr(), d_fc.data_ptr(), d_guide.data_ptr(), width,
                                  height, d_h[0].data_ptr(), d_h[1].data_ptr(), library=library, **uopts)
                d_motion = torch.from_numpy(motion.reshape(-1)).to(dev)   # (torch's allocations are 256-byte aligned)
                moved = dict(d_ids=d_ids.data_ptr(), d_motion=d_motion.data_ptr() if len(sc) else None, n_bodies=len(sc))
                if budget is not None:
                    tp.probe(cam, d_feat.data_ptr(), d_len.data_ptr(), **moved,
                             **{k: v for k, v in topts.items() if k != "clamp"})
                    bd.plan(d_len.data_ptr())
                    bd.trace(ds, cam, sample_begin=f * stride, fused=fused)
                    bd.resolve_half_into(d_h[0].data_ptr(), 0)
                    bd.resolve_half_into(d_h[1].data_ptr(), 1)
                    moved["d_mult"] = bd.d_mult
                tp.step(cam, d_h[0].data_ptr(), d_h[1].data_ptr(), d_feat.data_ptr(), d_acc[0].data_ptr(),
                        d_acc[1].data_ptr(), **moved, **topts)
                dn.run(d_acc[0].data_ptr(), d_acc[1].data_ptr(), d_guide.data_ptr(), d_out.data_ptr(), **opts)
                torch.cuda.synchronize(dev)
                if not refit:
                    ok(dll.rt_scene_free(ds))
                    ds = C.c_void_p()
                prev_sc = sc
                out = d_out.cpu().numpy().reshape(height, width, 3)
                if stages:
                    yield (out,) + tuple(d.cpu().numpy().reshape(height, width, 3) for d in d_h) + \
                        (d_feat.cpu().numpy().reshape(height, width, RT_FEAT_CHANNELS),) + \
                        tuple(d.cpu().numpy().reshape(height, width, 3) for d in d_acc) + \
                        (d_ids.cpu().numpy().reshape(height, width),) + ((bd.mult(),) if bd is not None else ()) + \
                        (() if scale is None else tuple(d.cpu().numpy().reshape(ch, cw, 3) for d in d_tr) +
                         (d_fc.cpu().numpy().reshape(ch, cw, RT_FEAT_CHANNELS),)) + \
                        (() if copt is None else (d_chain.cpu().numpy().reshape(height, width, RT_FEAT_CHANNELS),))
                else:
                    yield out
    finally:
        if bd is not None:
            bd.close()
        if ds:
            dll.rt_scene_free(ds)
        for a in acc:
            if a:
                dll.rt_accum_free(a)
        if ft:
            dll.rt_feat_free(ft)
        if fc:
            dll.rt_feat_free(fc)
        if fch:
            dll.rt_feat_free(fch)


def pass_sizes(spp: int, passes: int):
    """spp samples in `passes` near-equal passes (the larger ones first)."""
    k = max(1, min(int(passes), max(int(spp), 1)))
    return [spp // k + (1 if i < spp % k else 0) for i in range(k)]


def render(scene, cam: rt_camera, width: int, height: int, spp: int = 100, max_depth: int = 50, seed: int = 1,
           n_devices: int = 0, rows=None, sample_begin: int = 0, row_tile: int = 8, stats: dict | None = None,
           flags: int = 0, library=None, out=None, u8: bool = False, passes: int | None = None,
           adaptive: dict | None = None):
    """compute-pixel for every pixel of rows [r0, r1) (default: all), on the GPU.

    Returns float32 (rows, width, 3) linear RGB, each pixel the mean of its spp
    samples (raytracing.clj:155).  `scene` is a Scene or a list of bodies.
    `library`: another loaded build of the ABI (rtclj._lib.diag_lib()).
    `out`: a C-contiguous float32 (rows, width, 3) array to render into (a
    renderer drawing frames reuses its framebuffer; a fresh 10 MB array's
    pages are first touched by the copy into it).
    `u8`: return write-color!'s bytes instead (rt_render_u8: the frame is
    quantised on the device; bit-identical to write_color(render(...))).
    `passes`: render the spp in that many near-equal accumulating passes on
    device 0 (Progressive; the same bits as one launch; `stats` is not
    filled).
    `adaptive`: dict(tol_q16=, step=, min_spp=, max_spp=) -- sample adaptively
    on device 0 (Adaptive, run to the end; `spp` and `passes` are not read;
    with a dict `stats`, its "samples" and "tile_spp" are filled)."""
    dll = library if library is not None else lib
    if adaptive is not None or passes is not None:
        if n_devices not in (0, 1):
            raise ValueError("render: passes and adaptive sampling run on one device")
    if adaptive is not None:
        with Adaptive(scene, cam, width, height, max_depth=max_depth, seed=seed, rows=rows, row_tile=row_tile,
                      flags=flags, sample_begin=sample_begin, library=library, **adaptive) as ad:
            ad.run()
            got = ad.frame_u8() if u8 else ad.frame()
            if stats is not None:
                stats.update(samples=ad.samples_traced, tile_spp=ad.counts())
    elif passes is not None:
        with Progressive(scene, cam, width, height, max_depth, seed, rows=rows, row_tile=row_tile, flags=flags,
                         sample_begin=sample_begin, library=library) as pr:
            for n in pass_sizes(spp, passes):
                pr.add(n)
            got = pr.frame_u8() if u8 else pr.frame()
    if adaptive is not None or passes is not None:
        if out is None:
            return got
        if out.shape != got.shape or out.dtype != got.dtype:
            raise ValueError(f"render: out must be {got.dtype.name} {got.shape}")
        out[...] = got
        return out
    scene, p, out = _frame_args(scene, width, height, spp, max_depth, seed, n_devices, rows, sample_begin,
                                row_tile, flags, out, u8)
    st = rt_stats()
    if u8:
        code = dll.rt_render_u8(C.byref(scene.c), C.byref(cam), C.byref(p), u8ptr(out), out.size, C.byref(st))
    else:
        code = dll.rt_render(C.byref(scene.c), C.byref(cam), C.byref(p), fptr(out), out.size, C.byref(st))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    if stats is not None:
        stats.update(st.as_dict())
    return out


class Frame:
    """A frame in flight (rt_render_submit): wait() blocks until its rows are
    in the array and returns it.  Holds the scene, parameters and array until
    then; a frame dropped unwaited is waited on by its finaliser."""

    def __init__(self, dll, handle, keep, out):
        self._dll, self._h, self._keep, self.out = dll, handle, keep, out

    def wait(self, stats: dict | None = None):
        if self._h is None:
            raise RuntimeError("Frame.wait: already waited on")
        st = rt_stats()
        h, self._h = self._h, None
        code = self._dll.rt_render_wait(h, C.byref(st))
        self._keep = None
        if code < 0:
            raise RTError(code, self._dll.rt_last_error().decode(errors="replace"))
        if stats is not None:
            stats.update(st.as_dict())
        return self.out

    def __del__(self):
        if getattr(self, "_h", None) is not None:
            self._dll.rt_render_wait(self._h, None)


def render_async(scene, cam: rt_camera, width: int, height: int, spp: int = 100, max_depth: int = 50,
                 seed: int = 1, n_devices: int = 0, rows=None, sample_begin: int = 0, row_tile: int = 8,
                 flags: int = 0, library=None, out=None, u8: bool = False) -> Frame:
    """render(...) without waiting (rt_render_submit): the devices start on
    the frame and the call returns a Frame; several frames submitted before
    the first is waited on run concurrently.  The bits are render's."""
    dll = library if library is not None else lib
    scene, p, out = _frame_args(scene, width, height, spp, max_depth, seed, n_devices, rows, sample_begin,
                                row_tile, flags, out, u8)
    h = C.c_void_p()
    if u8:
        code = dll.rt_render_submit_u8(C.byref(scene.c), C.byref(cam), C.byref(p), u8ptr(out), out.size,
                                       C.byref(h))
    else:
        code = dll.rt_render_submit(C.byref(scene.c), C.byref(cam), C.byref(p), fptr(out), out.size, C.byref(h))
    if code < 0:
        raise RTError(code, dll.rt_last_error().decode(errors="replace"))
    return Frame(dll, h, (scene, cam, p), out)


def write_color(lin) -> np.ndarray:
    """write-color!'s channel mapping (raytracing.clj:19-26) -> uint8 array."""
    lin = np.ascontiguousarray(lin, np.float32)
    out = np.empty(lin.shape, np.uint8)
    check(lib.rt_quantize(fptr(lin), u8ptr(out), lin.size))
    return out


def write_ppm(path, rgb8) -> None:
    """PPM P3 as -main writes it (raytracing.clj:172-175)."""
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    h, w = rgb8.shape[:2]
    check(lib.rt_write_ppm(str(path).encode(), u8ptr(rgb8), w, h))


def write_png(path, rgb8) -> None:
    """The same pixels as write_ppm, as an 8-bit RGB PNG (rt_write_png; the
    format src/ppm2png.clj produces)."""
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    h, w = rgb8.shape[:2]
    check(lib.rt_write_png(str(path).encode(), u8ptr(rgb8), w, h))


def ppm_to_png(src, dst) -> None:
    """ppm2png/ppm->png (src/ppm2png.clj:35-87) via rt_ppm_to_png."""
    check(lib.rt_ppm_to_png(str(src).encode(), str(dst).encode()))


def read_ppm(path) -> np.ndarray:
    """Parse a P3 file (as written by write_ppm or the reference) -> uint8 (H, W, 3)."""
    tok = open(path).read().split()
    if tok[0] != "P3":
        raise ValueError(f"{path}: not a P3 PPM")
    w, h, mx = int(tok[1]), int(tok[2]), int(tok[3])
    if mx != 255:
        raise ValueError(f"{path}: max value {mx} != 255")
    return np.array(tok[4:4 + w * h * 3], np.int64).astype(np.uint8).reshape(h, w, 3)


def main(*args, out_path="scene.ppm", seed: int = 1, n_devices: int = 0, flags: int = 0) -> np.ndarray:
    """-main [spp] [depth] (raytracing.clj:95-177): render the five-body scene
    at 400 x 225 and write `out_path` (PPM P3).  Returns the uint8 image.
    flags: rt_params.flags (e.g. RT_FLAG_REJECTION_SAMPLERS)."""
    spp = int(args[0]) if len(args) > 0 and args[0] is not None else 100
    max_depth = int(args[1]) if len(args) > 1 and args[1] is not None else 50
    print("config:", {"samples-per-px": spp, "max-depth": max_depth})
    t0 = time.perf_counter()
    width = 400
    height = image_height(width)
    cam = camera(width, height, **REFERENCE_CAMERA)
    lin = render(hittables, cam, width, height, spp, max_depth, seed=seed, n_devices=n_devices, flags=flags)
    rgb = write_color(lin)
    write_ppm(out_path, rgb)
    print(f'"Elapsed time: {(time.perf_counter() - t0) * 1e3:.3f} msecs"')
    return rgb


if __name__ == "__main__":  # python -m rtclj.raytracing [spp] [depth]
    try:
        main(*sys.argv[1:3])
    except RTError as e:
        sys.exit(str(e))


__all__ = ["hittables", "REFERENCE_CAMERA", "image_height", "flatten", "flatten64", "Scene", "camera", "render", "Progressive", "Adaptive", "pass_sizes",
           "Features", "feat_chain_host", "denoise_host", "Denoiser", "render_denoised", "camera_coarsen", "coarse_size", "upsample_host", "upsample_into", "render_upscaled", "temporal_host", "Temporal", "temporal_probe_host", "budget_plan_host", "budget_units_host", "Budget", "render_sequence", "ids_host", "body_ids_into", "body_motion", "tree_build_host", "tree_refit_host", "tree_cost", "DeviceScene", "render_animation", "write_color", "write_ppm", "write_png", "ppm_to_png", "read_ppm", "main", "dptr"]
