"""ctypes binding of include/rt.h (librtclj.so).

This is the same binding a maintainer would add to the reference's host
(a JNI shim for Clojure); Python uses it for the tests,
bench.py and the Python host API.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG_ROOT = Path(__file__).resolve().parent.parent          # raytracing-clj_amd/
# RTCLJ_LIBRARY: load another build of the same ABI (A/B of kernel builds)
library_path = Path(os.environ["RTCLJ_LIBRARY"]) if os.environ.get("RTCLJ_LIBRARY") else _PKG_ROOT / "lib" / "librtclj.so"
# the diagnostic build (A/B and statistics kernel variants; same ABI)
diag_library_path = _PKG_ROOT / "lib" / "librtclj_diag.so"

RT_OK, RT_E_ARG, RT_E_MATERIAL, RT_E_TOO_MANY, RT_E_HIP, RT_E_NODEV, RT_E_IO = 0, -1, -2, -3, -4, -5, -6
RT_LAMBERTIAN, RT_METAL, RT_DIELECTRIC, RT_NONE = 0, 1, 2, 3
RT_MAX_SPHERES = 8192
RT_MAX_SPP = 1 << 24
RT_FLAG_SHARDS_ON_DEVICE0 = 1
RT_FLAG_REALM = 2
RT_FLAG_STREAMED = 4
RT_FLAG_REJECTION_SAMPLERS = 8   # vec3a.clj:74-86's rejection loops instead of the loop-free samplers


class RTError(RuntimeError):
    """A negative rt_status from the C ABI, with rt_last_error()'s message."""

    def __init__(self, code: int, message: str):
        super().__init__(f"rt error {code}: {message}")
        self.code = code


class rt_scene(C.Structure):
    _fields_ = [("n", C.c_int), ("sphere", C.POINTER(C.c_float)),
                ("mat_kind", C.POINTER(C.c_int)), ("mat", C.POINTER(C.c_float))]


class rt_camera(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("p00", C.c_float * 3), ("du", C.c_float * 3),
                ("dv", C.c_float * 3), ("disk_u", C.c_float * 3), ("disk_v", C.c_float * 3),
                ("defocus", C.c_int)]

    def as_list(self):
        """18 floats: center, p00, du, dv, disk_u, disk_v (the oracle's camera layout)."""
        out = []
        for f in ("center", "p00", "du", "dv", "disk_u", "disk_v"):
            out.extend(getattr(self, f))
        return out


class rt_params(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("row_begin", C.c_int), ("row_end", C.c_int),
                ("spp", C.c_int), ("max_depth", C.c_int), ("seed", C.c_uint64), ("sample_begin", C.c_int),
                ("n_devices", C.c_int), ("row_tile", C.c_int), ("tile_first", C.c_int),
                ("tile_step", C.c_int), ("flags", C.c_int)]


class rt_stats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("samples", C.c_uint64), ("kernel_ms", C.c_double),
                ("total_ms", C.c_double), ("n_devices", C.c_int), ("scene_cached", C.c_int),
                ("upload_ms", C.c_double), ("gather_ms", C.c_double), ("kernel_ms_mean", C.c_double),
                ("setup_ms", C.c_double), ("enqueue_ms", C.c_double), ("wait_ms", C.c_double),
                ("scatter_ms", C.c_double), ("other_ms", C.c_double), ("d2h_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class rt_adapt_opts(C.Structure):
    _fields_ = [("step_spp", C.c_int), ("min_spp", C.c_int), ("max_spp", C.c_int), ("tol_q16", C.c_uint32)]


class rt_denoise_opts(C.Structure):
    _fields_ = [("levels", C.c_int), ("normal_pow2", C.c_int), ("sigma_c", C.c_float), ("sigma_z", C.c_float)]


# rt_denoise's defaults (include/rt.h)
DENOISE_DEFAULTS = dict(levels=5, normal_pow2=5, sigma_c=4.0, sigma_z=0.05)


class rt_upsample_opts(C.Structure):
    _fields_ = [("scale", C.c_int), ("normal_pow2", C.c_int), ("sigma_z", C.c_float)]


class rt_feat_chain_opts(C.Structure):
    _fields_ = [("max_bounces", C.c_int), ("fuzz_max", C.c_float)]


class rt_chain_sample(C.Structure):
    _fields_ = [("body", C.c_int32), ("bounces", C.c_int32), ("length", C.c_float), ("albedo", C.c_float * 3),
                ("normal", C.c_float * 3)]


# rt_launch_feat_chain's defaults (include/rt.h)
CHAIN_DEFAULTS = dict(max_bounces=8, fuzz_max=0.0)
# rt_chain_sample as a NumPy record (36 bytes, no padding)
CHAIN_SAMPLE_DTYPE = [("body", "<i4"), ("bounces", "<i4"), ("length", "<f4"), ("albedo", "<f4", (3,)),
                      ("normal", "<f4", (3,))]


class rt_ray(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("t_min", C.c_float), ("d", C.c_float * 3), ("t_max", C.c_float)]


class rt_ray_hit(C.Structure):
    _fields_ = [("body", C.c_int32), ("front_face", C.c_int32), ("t", C.c_float), ("dist", C.c_float),
                ("normal", C.c_float * 3), ("reserved", C.c_float)]


# rt_ray and rt_ray_hit as NumPy records (32 bytes each, no padding)
RAY_DTYPE = [("o", "<f4", (3,)), ("t_min", "<f4"), ("d", "<f4", (3,)), ("t_max", "<f4")]
RAY_HIT_DTYPE = [("body", "<i4"), ("front_face", "<i4"), ("t", "<f4"), ("dist", "<f4"), ("normal", "<f4", (3,)),
                 ("reserved", "<f4")]


# rt_upsample's defaults (include/rt.h)
UPSAMPLE_DEFAULTS = dict(scale=2, normal_pow2=0, sigma_z=0.05)


class rt_temporal_opts(C.Structure):
    _fields_ = [("max_history", C.c_int), ("sigma_z", C.c_float), ("normal_min", C.c_float)]


class rt_temporal_clamp_opts(C.Structure):
    _fields_ = [("radius", C.c_int), ("gamma", C.c_float)]


class rt_budget_opts(C.Structure):
    _fields_ = [("half_spp", C.c_int), ("target", C.c_int), ("max_mult", C.c_int), ("quantile_64", C.c_int)]


class rt_tree_info(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("off_pairs", C.c_int), ("off_pidx", C.c_int), ("blob_bytes", C.c_int),
                ("big_pair0", C.c_int), ("n_big_leaves", C.c_int), ("depth", C.c_int), ("leaf_size", C.c_int),
                ("idx_bytes", C.c_int), ("center", C.c_float * 3), ("radius", C.c_float), ("c0", C.c_float)]

    def as_dict(self):
        return {f: (tuple(getattr(self, f)) if f == "center" else getattr(self, f)) for f, _ in self._fields_}


class rt_schedule_info(C.Structure):
    _fields_ = [("exists", C.c_int32), ("n_tiles", C.c_int32), ("has_record", C.c_int32), ("ready", C.c_int32),
                ("sort_pending", C.c_int32), ("plan_units", C.c_int32), ("sort_plan", C.c_int32),
                ("max_streams", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# rt_temporal_step's defaults (include/rt.h)
TEMPORAL_DEFAULTS = dict(max_history=32, sigma_z=0.1, normal_min=0.9)
# rt_temporal_step_clamp's defaults (include/rt.h)
TEMPORAL_CLAMP_DEFAULTS = dict(radius=2, gamma=1.0)
# rt_budget_opts' defaults (include/rt.h); half_spp has none
BUDGET_DEFAULTS = dict(target=8, max_mult=8, quantile_64=16)


# symbol -> (restype, argtypes); every function include/rt.h declares
SIGNATURES = {
    "rt_camera_setup": (C.c_int, [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(rt_camera)]),
    "rt_camera_coarsen": (C.c_int, [C.POINTER(rt_camera), C.c_int, C.POINTER(rt_camera)]),
    "rt_upsample": (C.c_int, [C.POINTER(rt_upsample_opts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_upsample_host": (C.c_int, [C.POINTER(rt_upsample_opts)] + [C.POINTER(C.c_float)] * 4 + [C.c_int, C.c_int] +
                         [C.POINTER(C.c_float)] * 2),
    "rt_quantize": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_size_t]),
    "rt_write_ppm": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint8), C.c_int, C.c_int]),
    "rt_write_png": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint8), C.c_int, C.c_int]),
    "rt_ppm_to_png": (C.c_int, [C.c_char_p, C.c_char_p]),
    "rt_rows_out": (C.c_int, [C.POINTER(rt_params)]),
    "rt_prepare": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "rt_scene_reference": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]),
    "rt_scene_cover": (C.c_int, [C.c_int, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_int),
                                 C.POINTER(C.c_float), C.c_int]),
    "rt_render": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_camera), C.POINTER(rt_params),
                            C.POINTER(C.c_float), C.c_size_t, C.POINTER(rt_stats)]),
    "rt_render_u8": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_camera), C.POINTER(rt_params),
                               C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(rt_stats)]),
    "rt_render_submit": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_camera), C.POINTER(rt_params),
                                   C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_void_p)]),
    "rt_render_submit_u8": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_camera), C.POINTER(rt_params),
                                      C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_void_p)]),
    "rt_render_wait": (C.c_int, [C.c_void_p, C.POINTER(rt_stats)]),
    "rt_cache_clear": (C.c_int, []),
    "rt_scene_upload": (C.c_int, [C.c_int, C.POINTER(rt_scene), C.POINTER(C.c_void_p)]),
    "rt_scene_free": (C.c_int, [C.c_void_p]),
    "rt_launch": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_void_p,
                            C.c_void_p, C.c_void_p]),
    "rt_accum_create": (C.c_int, [C.c_void_p, C.POINTER(rt_params), C.POINTER(C.c_void_p)]),
    "rt_accum_free": (C.c_int, [C.c_void_p]),
    "rt_accum_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_accum_samples": (C.c_int64, [C.c_void_p]),
    "rt_launch_accum": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "rt_accum_resolve": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_accum_resolve_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_accum_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "rt_accum_add": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64, C.c_void_p]),
    "rt_resolve_sums": (C.c_int, [C.POINTER(C.c_uint64), C.c_size_t, C.c_int64, C.c_int, C.POINTER(C.c_float)]),
    "rt_adapt_create": (C.c_int, [C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_adapt_opts), C.POINTER(C.c_void_p)]),
    "rt_adapt_free": (C.c_int, [C.c_void_p]),
    "rt_adapt_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_adapt_step": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "rt_adapt_active": (C.c_int, [C.c_void_p]),
    "rt_adapt_samples": (C.c_int64, [C.c_void_p]),
    "rt_adapt_resolve": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_adapt_resolve_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_adapt_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "rt_adapt_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]),
    "rt_adapt_eval_host": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_uint32,
                                     C.POINTER(C.c_uint8)]),
    "rt_adapt_resolve_host": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int,
                                        C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "rt_feat_create": (C.c_int, [C.c_void_p, C.POINTER(rt_params), C.POINTER(C.c_void_p)]),
    "rt_feat_free": (C.c_int, [C.c_void_p]),
    "rt_feat_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_feat_samples": (C.c_int64, [C.c_void_p]),
    "rt_launch_feat": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "rt_feat_resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_feat_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                               C.c_void_p]),
    "rt_feat_add": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                              C.c_int64, C.c_void_p]),
    "rt_feat_resolve_host": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_size_t,
                                       C.c_int64, C.POINTER(C.c_float)]),
    "rt_feat_occupancy": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rt_launch_feat_chain": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params),
                                       C.POINTER(rt_feat_chain_opts), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_feat_chain_host": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_feat_chain_opts), C.POINTER(C.c_float),
                                     C.c_size_t, C.POINTER(rt_chain_sample)]),
    "rt_feat_chain_occupancy": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rt_adapt_resolve_half": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_denoiser_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rt_denoiser_free": (C.c_int, [C.c_void_p]),
    "rt_denoise": (C.c_int, [C.c_void_p, C.POINTER(rt_denoise_opts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p]),
    "rt_denoise_profile": (C.c_int, [C.c_void_p, C.POINTER(rt_denoise_opts), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "rt_denoise_host": (C.c_int, [C.POINTER(rt_denoise_opts), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "rt_temporal_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rt_temporal_free": (C.c_int, [C.c_void_p]),
    "rt_temporal_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_temporal_frames": (C.c_int64, [C.c_void_p]),
    "rt_temporal_step": (C.c_int, [C.c_void_p, C.POINTER(rt_temporal_opts), C.POINTER(rt_camera), C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_temporal_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.POINTER(C.c_float), C.c_void_p]),
    "rt_temporal_host": (C.c_int, [C.POINTER(rt_temporal_opts), C.POINTER(rt_camera), C.POINTER(rt_camera), C.c_int,
                                   C.c_int, C.c_int] + [C.POINTER(C.c_float)] * 10),
    "rt_temporal_step_motion": (C.c_int, [C.c_void_p, C.POINTER(rt_temporal_opts), C.POINTER(rt_camera), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "rt_temporal_host_motion": (C.c_int, [C.POINTER(rt_temporal_opts), C.POINTER(rt_camera), C.POINTER(rt_camera),
                                          C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_float)] * 7 +
                                [C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int] + [C.POINTER(C.c_float)] * 3),
    "rt_temporal_step_clamp": (C.c_int, [C.c_void_p, C.POINTER(rt_temporal_opts), C.POINTER(rt_temporal_clamp_opts),
                                         C.POINTER(rt_camera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_temporal_host_clamp": (C.c_int, [C.POINTER(rt_temporal_opts), C.POINTER(rt_temporal_clamp_opts),
                                         C.POINTER(rt_camera), C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int] +
                               [C.POINTER(C.c_float)] * 7 + [C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int] +
                               [C.POINTER(C.c_float)] * 3),
    "rt_temporal_probe": (C.c_int, [C.c_void_p, C.POINTER(rt_temporal_opts), C.POINTER(rt_camera), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_temporal_host_probe": (C.c_int, [C.POINTER(rt_temporal_opts), C.POINTER(rt_camera), C.POINTER(rt_camera),
                                         C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_float)] * 3 +
                               [C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float)]),
    "rt_budget_plan_host": (C.c_int, [C.POINTER(rt_budget_opts), C.POINTER(C.c_float), C.c_int, C.c_int,
                                      C.POINTER(C.c_uint32)]),
    "rt_budget_create": (C.c_int, [C.c_void_p, C.POINTER(rt_params), C.POINTER(rt_budget_opts),
                                   C.POINTER(C.c_void_p)]),
    "rt_budget_free": (C.c_int, [C.c_void_p]),
    "rt_budget_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_budget_plan_mult": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_budget_trace": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "rt_budget_trace_fused": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_params), C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "rt_budget_units_host": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_int32)]),
    "rt_budget_units_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_void_p]),
    "rt_budget_list_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "rt_budget_resolve": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_budget_resolve_half": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_budget_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]),
    "rt_budget_mult_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "rt_budget_device_mult": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rt_budget_samples": (C.c_int64, [C.c_void_p]),
    "rt_temporal_step_budget": (C.c_int, [C.c_void_p, C.POINTER(rt_temporal_opts), C.POINTER(rt_temporal_clamp_opts),
                                          C.POINTER(rt_camera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_temporal_host_budget": (C.c_int, [C.POINTER(rt_temporal_opts), C.POINTER(rt_temporal_clamp_opts),
                                          C.POINTER(rt_camera), C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int] +
                                [C.POINTER(C.c_float)] * 7 + [C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int,
                                                              C.POINTER(C.c_uint32)] + [C.POINTER(C.c_float)] * 3),
    "rt_launch_ids": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_ids_host": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int,
                              C.POINTER(C.c_int32)]),
    "rt_ids_occupancy": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rt_body_motion": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_scene), C.POINTER(C.c_float)]),
    "rt_launch_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rt_launch_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rt_rays_host": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_ray), C.POINTER(C.c_int32), C.c_size_t,
                               C.POINTER(rt_ray_hit)]),
    "rt_occluded_host": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_ray), C.POINTER(C.c_int32), C.c_size_t,
                                   C.POINTER(C.c_uint8)]),
    "rt_rays_occupancy": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rt_scene_update": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_void_p]),
    "rt_tree_build_host": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                     C.POINTER(rt_tree_info)]),
    "rt_tree_refit_host": (C.c_int, [C.c_void_p, C.POINTER(rt_tree_info), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.c_int]),
    "rt_tree_cost_host": (C.c_int, [C.c_void_p, C.POINTER(rt_tree_info), C.POINTER(C.c_double)]),
    "rt_scene_tree_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rt_tree_info)]),
    "rt_scene_tree_read": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_quantize_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_set_variant": (C.c_int, [C.c_int]),
    "rt_resolve_variant": (C.c_int, [C.c_void_p]),
    "rt_launch_occupancy": (C.c_int, [C.c_void_p, C.POINTER(rt_params), C.POINTER(C.c_int)]),
    "rt_set_schedule": (C.c_int, [C.c_int]),
    "rt_debug_stats": (C.c_int, [C.POINTER(C.c_uint64)]),
    "rt_debug_stats_ext": (C.c_int, [C.POINTER(C.c_uint64), C.c_int]),
    "rt_tile_bodies_host": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_camera), C.POINTER(rt_params), C.c_int,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    "rt_debug_waves": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.c_size_t]),
    "rt_steal_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_export_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_schedule_read": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(rt_schedule_info), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "rt_schedule_sort": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                   C.POINTER(C.c_int32), C.c_void_p]),
    "rt_device_count": (C.c_int, []),
    "rt_last_error": (C.c_char_p, []),
    "rt_version": (C.c_char_p, []),
    "rt_abi_version": (C.c_int, []),
}

RT_ABI_VERSION = 3   # include/rt.h; the structures above are this revision's
# functions added within the revision (a build from before them still loads)
ADDITIVE = {"rt_prepare", "rt_render_u8", "rt_quantize_device", "rt_render_submit", "rt_render_submit_u8",
            "rt_render_wait", "rt_export_stats", "rt_accum_create", "rt_accum_free", "rt_accum_clear",
            "rt_accum_samples", "rt_launch_accum", "rt_accum_resolve", "rt_accum_resolve_u8", "rt_accum_read",
            "rt_accum_add", "rt_resolve_sums", "rt_adapt_create", "rt_adapt_free", "rt_adapt_clear", "rt_adapt_step",
            "rt_adapt_active", "rt_adapt_samples", "rt_adapt_resolve", "rt_adapt_resolve_u8", "rt_adapt_counts",
            "rt_adapt_read", "rt_adapt_eval_host", "rt_adapt_resolve_host", "rt_feat_create", "rt_feat_free",
            "rt_feat_clear", "rt_feat_samples", "rt_launch_feat", "rt_feat_resolve", "rt_feat_read",
            "rt_feat_add", "rt_feat_resolve_host", "rt_feat_occupancy", "rt_adapt_resolve_half",
            "rt_denoiser_create", "rt_denoiser_free", "rt_denoise", "rt_denoise_profile",
            "rt_denoise_host", "rt_temporal_create", "rt_temporal_free", "rt_temporal_reset", "rt_temporal_frames",
            "rt_temporal_step", "rt_temporal_read", "rt_temporal_host", "rt_temporal_step_motion",
            "rt_temporal_host_motion", "rt_temporal_step_clamp", "rt_temporal_host_clamp", "rt_temporal_probe",
            "rt_temporal_host_probe", "rt_budget_plan_host", "rt_budget_create", "rt_budget_free", "rt_budget_plan",
            "rt_budget_plan_mult", "rt_budget_trace", "rt_budget_resolve", "rt_budget_resolve_half", "rt_budget_read",
            "rt_budget_mult_read", "rt_budget_device_mult", "rt_budget_samples", "rt_temporal_step_budget",
            "rt_temporal_host_budget", "rt_launch_ids", "rt_ids_host", "rt_ids_occupancy", "rt_body_motion",
            "rt_scene_update", "rt_tree_build_host", "rt_tree_refit_host", "rt_tree_cost_host", "rt_scene_tree_info",
            "rt_scene_tree_read", "rt_schedule_read", "rt_schedule_sort", "rt_camera_coarsen", "rt_upsample",
            "rt_upsample_host", "rt_launch_feat_chain", "rt_feat_chain_host", "rt_feat_chain_occupancy",
            "rt_budget_trace_fused", "rt_budget_units_host", "rt_budget_units_read", "rt_budget_list_read",
            "rt_debug_stats_ext", "rt_tile_bodies_host", "rt_launch_rays", "rt_launch_occluded", "rt_rays_host",
            "rt_occluded_host", "rt_rays_occupancy"}

RT_FEAT_CHANNELS = 8   # rt_feat_resolve's floats per pixel: albedo rgb, normal xyz, depth, coverage


def load(path: Path) -> C.CDLL:
    """Load a build of include/rt.h's ABI with every signature bound.  Local
    binding (RTLD_LOCAL; the library exports only rt_* symbols): the product
    and the diagnostic build can be loaded side by side."""
    if not Path(path).exists():
        raise ImportError(f"{path} is missing: build it with `make -C {_PKG_ROOT}` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    dll = C.CDLL(str(path), mode=os.RTLD_NOW | os.RTLD_LOCAL)
    for name, (res, args) in SIGNATURES.items():
        if name in ADDITIVE and not hasattr(dll, name):
            continue   # (an older build of the same revision: A/B of library builds)
        fn = getattr(dll, name)
        fn.restype = res
        fn.argtypes = args
    if dll.rt_abi_version() != RT_ABI_VERSION:
        raise ImportError(f"{path}: ABI revision {dll.rt_abi_version()}, this binding is {RT_ABI_VERSION} "
                          "(rebuild the library: make -C raytracing-clj_amd)")
    return dll


lib = load(library_path)
_diag = None


def diag_lib() -> C.CDLL:
    """The diagnostic build (lib/librtclj_diag.so: the A/B and statistics
    kernel variants, rt_set_variant 1-19), loaded on first use."""
    global _diag
    if _diag is None:
        _diag = load(diag_library_path)
    return _diag


def check(code: int) -> int:
    """Raise RTError for a negative status, else return it."""
    if code < 0:
        raise RTError(code, lib.rt_last_error().decode(errors="replace"))
    return code


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def i32ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def u8ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def u32ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def u64ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def i64ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))
