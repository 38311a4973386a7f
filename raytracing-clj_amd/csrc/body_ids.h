// body_ids.h — the body-id pass (rt_launch_ids, rt_ids_host, include/rt.h):
// which body the pixel centre's pinhole ray meets first, as its index in the
// scene's array order, and the per-body displacement between two scenes
// (rt_body_motion) that the motion-aware temporal step subtracts (temporal.h).
//
// Replaces nothing the reference computes on its own: it exposes the index
// hit-anything's reduce (src/raytracing.clj:33-43) ends on and drops, for
// compute-pixel's ray (src/raytracing.clj:144-151) without its jitter.
//
// Three parts, as first_hit.h, denoise.h and temporal.h.
//  1. One pixel as plain inline functions that compile for the device (the
//     kernel below) and for the host (rt_ids_host, tools/motion_check.cpp): the
//     ray of temporal.h's step 1, then first_hit.h's search -- no text of its
//     own for the body test, the acceptance or the walk.
//  2. The pass and the displacement on the host, checks included
//     (ids_host_pass, body_motion): what rt_ids_host and rt_body_motion run,
//     and what tools/motion_check.cpp runs under the sanitizers.
//  3. The device kernel (under __HIPCC__ and RT_BODY_IDS_KERNEL, after
//     first_hit.h's kernel part): one thread per pixel, one ray a thread, no
//     atomics, no scratch, one 4-byte store.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rt.h"
#include "first_hit.h"
#include "temporal.h"

namespace rtclj {

// ------------------------------------------------------------ one pixel ----
// temporal.h's step 1: e_c = ((p00_c + float(x) du_c) + float(j) dv_c) - center_c,
// every operation rounded once (no fma: built with -ffp-contract=off).
// cam12 = center, p00, du, dv.
RT_FH_FN void ids_ray_dir(const float* cam12, int x, int j, float* e) {
  const float xf = static_cast<float>(x), jf = static_cast<float>(j);
  for (int c = 0; c < 3; ++c) e[c] = ((cam12[3 + c] + xf * cam12[6 + c]) + jf * cam12[9 + c]) - cam12[c];
}
RT_FH_FN FhRay ids_ray(const float* cam12, int x, int j) {
  float e[3];
  ids_ray_dir(cam12, x, j, e);
  return fh_ray(cam12[0], cam12[1], cam12[2], e[0], e[1], e[2]);
}

// ------------------------------------------------------------- the host ----
inline void ids_cam12(const rt_camera& c, float* cam12) {
  for (int k = 0; k < 3; ++k) {
    cam12[k] = c.center[k];
    cam12[3 + k] = c.p00[k];
    cam12[6 + k] = c.du[k];
    cam12[9 + k] = c.dv[k];
  }
}

// rt_ids_host (rt.h): the checks, then fh_scan over fh_geo's table for every
// pixel.  0, or RT_E_ARG with *why set.
inline int ids_host_pass(const rt_scene* s, const rt_camera* c, int width, int rows, int row0, int32_t* out,
                         const char** why) {
  *why = nullptr;
  if (!s || !c || !out) {
    *why = "NULL argument";
    return RT_E_ARG;
  }
  if (s->n < 0 || (s->n > 0 && !s->sphere)) {
    *why = "bad scene arrays";
    return RT_E_ARG;
  }
  if ((*why = tp_shape_error(width, rows, row0)) != nullptr) return RT_E_ARG;
  std::vector<float> geo(4 * static_cast<size_t>(s->n));
  for (int b = 0; b < s->n; ++b) fh_geo(s->sphere + 4 * static_cast<size_t>(b), &geo[4 * static_cast<size_t>(b)]);
  float cam12[12];
  ids_cam12(*c, cam12);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < width; ++x) {
      const FhRay r = ids_ray(cam12, x, row0 + y);
      FhBest best = fh_none();
      fh_scan(r, geo.data(), s->n, best);
      out[static_cast<size_t>(y) * width + x] = best.body;
    }
  return RT_OK;
}

// rt_body_motion (rt.h): out[4 b + c] = cur.center_c - prev.center_c, lane 3 = 0;
// a body whose radius, kind or material differs by bits has no past: NaN.
inline int body_motion(const rt_scene* cur, const rt_scene* prev, float* out, const char** why) {
  *why = nullptr;
  if (!cur || !prev || !out) {
    *why = "NULL argument";
    return RT_E_ARG;
  }
  if (cur->n < 0 || cur->n != prev->n) {
    *why = "the scenes' body counts differ";
    return RT_E_ARG;
  }
  for (const rt_scene* s : {cur, prev})
    if (s->n > 0 && (!s->sphere || !s->mat_kind || !s->mat)) {
      *why = "bad scene arrays";
      return RT_E_ARG;
    }
  for (int b = 0; b < cur->n; ++b) {
    const float *sc = cur->sphere + 4 * static_cast<size_t>(b), *sp = prev->sphere + 4 * static_cast<size_t>(b);
    const bool same = std::memcmp(sc + 3, sp + 3, sizeof(float)) == 0 && cur->mat_kind[b] == prev->mat_kind[b] &&
                      std::memcmp(cur->mat + 4 * static_cast<size_t>(b), prev->mat + 4 * static_cast<size_t>(b),
                                  4 * sizeof(float)) == 0;
    float* o = out + 4 * static_cast<size_t>(b);
    for (int c = 0; c < 3; ++c) o[c] = same ? sc[c] - sp[c] : NAN;
    o[3] = 0.0f;
  }
  return RT_OK;
}

#if defined(__HIPCC__) && defined(RT_BODY_IDS_KERNEL) && defined(RT_FIRST_HIT_KERNEL)
// ----------------------------------------------------------- the kernel ----
struct alignas(16) IdsArgs {
  const float4* geo;    // n: cx, cy, cz, -r^2 (the scan)
  const float4* blob;   // the tree (FEAT_LDS, FEAT_GLOBAL)
  int blob_f4, off_pairs, off_pidx, leaf_pairs, big_pair0, n_big_leaves, ref_mul;
  float bvh_c[3], bvh_r, bvh_c0;
  float cam[12];        // center, p00, du, dv
  int n, width, rows, row0;
  int32_t* ids;         // rows x width
};

// A workgroup is kDnBx x kDnBy pixels, a wave one row of 64 (the denoiser's
// and the temporal step's shape); thread (x, y) owns pixel (x, y) and traces
// its one ray.  SRC as feat_kernel's: the tree's image staged in LDS by the
// whole workgroup, the tree read from global memory, or the linear scan; the
// walk stack is FhLdsStack's u16 [entry][lane] rows behind the image either
// way.  A thread outside the image leaves after the staging.
template <int SRC>
__global__ __launch_bounds__(kDnBx* kDnBy) void ids_kernel(const IdsArgs a) {
  static_assert(kDnBx * kDnBy == kFeatThreads, "FhLdsStack's row length");
  extern __shared__ __attribute__((aligned(16))) float4 s_ids_img[];   // the tree's blob, then the stack rows
  const int t = static_cast<int>(threadIdx.y) * kDnBx + static_cast<int>(threadIdx.x);
  if constexpr (SRC == FEAT_LDS) {
    for (int i = t; i < a.blob_f4; i += kFeatThreads) s_ids_img[i] = a.blob[i];
    __syncthreads();
  }
  const int x = static_cast<int>(blockIdx.x) * kDnBx + static_cast<int>(threadIdx.x);
  const int y = static_cast<int>(blockIdx.y) * kDnBy + static_cast<int>(threadIdx.y);
  if (x >= a.width || y >= a.rows) return;
  const FhRay r = ids_ray(a.cam, x, a.row0 + y);
  FhBest best = fh_none();
  if constexpr (SRC == FEAT_SCAN) {
    fh_scan(r, reinterpret_cast<const float*>(a.geo), a.n, best);
  } else {
    FhTree tr;
    tr.base = SRC == FEAT_LDS ? reinterpret_cast<const char*>(s_ids_img) : reinterpret_cast<const char*>(a.blob);
    tr.off_pairs = a.off_pairs, tr.off_pidx = a.off_pidx, tr.leaf_pairs = a.leaf_pairs;
    tr.big_pair0 = a.big_pair0, tr.n_big_leaves = a.n_big_leaves, tr.ref_mul = a.ref_mul;
    tr.c[0] = a.bvh_c[0], tr.c[1] = a.bvh_c[1], tr.c[2] = a.bvh_c[2], tr.r = a.bvh_r, tr.c0 = a.bvh_c0;
    unsigned short* stack0 = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(s_ids_img) +
                                                               (SRC == FEAT_LDS ? a.blob_f4 * 16 : 0));
    FhLdsStack stk{stack0 + t, 0};
    fh_walk(r, tr, stk, best);
  }
  a.ids[static_cast<size_t>(y) * a.width + x] = best.body;
}
#endif  // __HIPCC__ && RT_BODY_IDS_KERNEL

}  // namespace rtclj
