// ray_query.h — ray queries (rt_launch_rays, rt_launch_occluded, rt_rays_host,
// rt_occluded_host, include/rt.h): the closest hit, or whether there is any,
// for rays the caller brings, against the scene the renderer traces.
//
// Replaces nothing the reference computes on its own: it exposes hit-anything
// (src/raytracing.clj:33-43) over the sphere ::hit-fn (src/hittable.clj:7-31,
// hit.clj:14-15) for a ray that does not come from compute-pixel.
//
// Three parts, as body_ids.h.
//  1. One ray as plain inline functions that compile for the device (the
//     kernels below) and for the host (rt_rays_host, rt_occluded_host,
//     tools/rays_check.cpp): the set-up and the inactive test of rt.h's steps 1
//     and 2, then first_hit.h's search with the self-hit guard (no text of its
//     own for the body test, the acceptance or the walk), then the record,
//     whose normal is rebuilt around the ray's closest point to the centre.
//  2. The passes on the host, checks included (rays_host_pass,
//     occluded_host_pass): what the host entries run, and what
//     tools/rays_check.cpp runs under the sanitizers.
//  3. The device kernels (under __HIPCC__ and RT_RAY_QUERY_KERNEL, after
//     first_hit.h's kernel part): one ray a thread, grid-stride over blocks of
//     256 rays, no atomics, no scratch.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/rt.h"
#include "first_hit.h"

namespace rtclj {

// -------------------------------------------------------------- one ray ----
// rt.h's steps 1 and 2: fh_ray's |d|, 1 / |d| and u; tmin = t_min * |d| (with
// t_min = 1e-3f fh_ray's own product); tbest = t_max * |d|, where the search
// starts.  false: the ray is inactive and must not reach the search (the
// walk's cull takes tmin < tbest for granted).
RT_FH_FN bool rq_ray(float ox, float oy, float oz, float t_min, float dx, float dy, float dz, float t_max, FhRay& r,
                     float& tbest) {
  r = fh_ray(ox, oy, oz, dx, dy, dz);
  r.tmin = t_min * r.len;
  tbest = t_max * r.len;
  const bool origin = fabsf(ox) < INFINITY && fabsf(oy) < INFINITY && fabsf(oz) < INFINITY;
  const bool length = r.len > 0.0f && r.len < INFINITY;
  const bool bounds = t_min >= 0.0f && t_max > t_min;
  return origin && length && bounds && r.tmin < tbest;
}

// rt.h's step 3: the body `last` names for the self-hit guard, or -1.  The guard
// puts |h| in sqrt(disc)'s place, so it would find a root on a body that has no
// disc -- a NaN or infinite centre or radius, an r * r that overflows -- which
// the scan otherwise never hits and the tree does not hold.  Such a body, like
// an index outside [0, n), is no guard.  geo: the scan's table (centre, -r^2).
RT_FH_FN int rq_guard(const float* geo, int n, int last) {
  if (last < 0 || last >= n) return -1;
  const float* g = geo + 4 * static_cast<size_t>(last);
  const bool finite = fabsf(g[0]) < INFINITY && fabsf(g[1]) < INFINITY && fabsf(g[2]) < INFINITY && fabsf(g[3]) < INFINITY;
  return finite ? last : -1;
}

// a record's eight words, as two 16-byte halves (the kernel's two stores)
struct RqHit {
  int body, front;
  float t, dist, nx, ny, nz, reserved;
};
RT_FH_FN RqHit rq_none() { return RqHit{-1, 0, INFINITY, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f}; }

// rt.h's step 4: the record of the closest hit `best` of r = rq_ray(o, d); sph4 =
// the body's (cx, cy, cz, 1 / r), rt_scene_upload's table, r2 its r * r (the
// scan's table holds -r^2).
// The normal is not taken from P = o + dist u.  The scan's disc = h^2 - (|oc|^2
// - r^2) cancels at the size of |oc|^2, so on a small far body the root is off
// by up to 6e-4 (|oc| + r) (bvh_pad.h) and (P - C) / r by that over r: 8e-3 on
// an r = 0.2 body 27 units away, which is nothing to a depth buffer but is to a
// caller that reflects, shades or resolves a collision with the normal.  It is
// rebuilt around the ray's closest point to the centre instead (Haines et al.,
// "Precision improvements for ray/sphere intersection", Ray Tracing Gems 7):
//   w = oc - h u, the part of oc across the ray (one fma a component: h's own
//       error lies along u and drops out of |w| to first order),
//   s = sqrt(max(r^2 - |w|^2, 0)): half the chord, from numbers of the size of r,
//   P - C = (h -+ s) u - oc = -+ s u - w, the sign by which root `dist` is
//       (the nearer one iff dist <= h; the guard's 2 h is the farther one).
// Then hit.clj:14-15 as the feature sample reads it: front iff dot(d, n) < 0
// on the un-normalised d, n turned against d, one correctly rounded 1 / |n|.
// A NaN component (a body of radius 0 met in its centre) is stored as 0, what
// rt_feat's conversion makes of it.
RT_FH_FN RqHit rq_record(const FhRay& r, const FhBest& best, float dx, float dy, float dz, const float* sph4, float r2) {
  RqHit h;
  h.body = best.body;
  h.dist = best.t;
  h.t = best.t * fh_rcp(r.len);
  const float ocx = sph4[0] - r.ox, ocy = sph4[1] - r.oy, ocz = sph4[2] - r.oz;
  const float hh = fmaf(r.uz, ocz, fmaf(r.uy, ocy, r.ux * ocx));   // fh_test's h
  const float wx = fmaf(-hh, r.ux, ocx), wy = fmaf(-hh, r.uy, ocy), wz = fmaf(-hh, r.uz, ocz);
  const float s = fh_sqrt(fmaxf(r2 - fmaf(wz, wz, fmaf(wy, wy, wx * wx)), 0.0f));
  const float ss = best.t > hh ? s : -s;
  float nx = fmaf(ss, r.ux, -wx) * sph4[3], ny = fmaf(ss, r.uy, -wy) * sph4[3], nz = fmaf(ss, r.uz, -wz) * sph4[3];
  const bool front = fmaf(dz, nz, fmaf(dy, ny, dx * nx)) < 0.0f;
  if (!front) {
    nx = -nx;
    ny = -ny;
    nz = -nz;
  }
  const float nil = fh_rcp(fh_sqrt(fmaf(nz, nz, fmaf(ny, ny, nx * nx))));
  nx = nx * nil;
  ny = ny * nil;
  nz = nz * nil;
  h.front = front ? 1 : 0;
  h.nx = nx == nx ? nx : 0.0f;
  h.ny = ny == ny ? ny : 0.0f;
  h.nz = nz == nz ? nz : 0.0f;
  h.reserved = 0.0f;
  return h;
}

// rt.h's step 5 over the scan's table: fh_scan from {tbest, -1}, left at the
// first body the test accepts
RT_FH_FN bool rq_scan_any(const FhRay& r, const float* geo, int n, float tbest, int last) {
  FhBest b{tbest, -1};
  for (int s = 0; s < n; ++s) {
    fh_test<true>(r, geo[4 * s], geo[4 * s + 1], geo[4 * s + 2], geo[4 * s + 3], s, b, last);
    if (b.body >= 0) return true;
  }
  return false;
}

// ------------------------------------------------------------- the host ----
inline const char* rq_args_error(const rt_scene* s, const void* rays, size_t n, const void* out) {
  if (!s || (n > 0 && (!rays || !out))) return "NULL argument";
  if (s->n < 0 || (s->n > 0 && !s->sphere)) return "bad scene arrays";
  if (n > 0x7fffffffu) return "more than 2^31 - 1 rays";
  return nullptr;
}
// the scan's table (fh_geo) and the normals' (centre, 1 / r: rt_scene_upload's division)
inline void rq_tables(const rt_scene& s, std::vector<float>* geo, std::vector<float>* sph) {
  const size_t nb = static_cast<size_t>(s.n);
  geo->resize(4 * nb);
  if (sph) sph->resize(4 * nb);
  for (size_t b = 0; b < nb; ++b) {
    const float* q = s.sphere + 4 * b;
    fh_geo(q, geo->data() + 4 * b);
    if (sph) {
      float* p = sph->data() + 4 * b;
      p[0] = q[0], p[1] = q[1], p[2] = q[2], p[3] = 1.0f / q[3];
    }
  }
}

// rt_rays_host (rt.h): the checks, then per ray the guarded scan over fh_geo's
// table and the record.  0, or RT_E_ARG with *why set.
inline int rays_host_pass(const rt_scene* s, const rt_ray* rays, const int32_t* last, size_t n, rt_ray_hit* out,
                          const char** why) {
  if ((*why = rq_args_error(s, rays, n, out)) != nullptr) return RT_E_ARG;
  std::vector<float> geo, sph;
  rq_tables(*s, &geo, &sph);
  for (size_t i = 0; i < n; ++i) {
    const rt_ray& q = rays[i];
    FhRay r;
    float tbest;
    RqHit h = rq_none();
    if (rq_ray(q.o[0], q.o[1], q.o[2], q.t_min, q.d[0], q.d[1], q.d[2], q.t_max, r, tbest)) {
      FhBest best{tbest, -1};
      fh_scan<true>(r, geo.data(), s->n, best, last ? rq_guard(geo.data(), s->n, last[i]) : -1);
      if (best.body >= 0) {
        const size_t k = 4 * static_cast<size_t>(best.body);
        h = rq_record(r, best, q.d[0], q.d[1], q.d[2], &sph[k], -geo[k + 3]);
      }
    }
    rt_ray_hit& o = out[i];
    o.body = h.body, o.front_face = h.front, o.t = h.t, o.dist = h.dist;
    o.normal[0] = h.nx, o.normal[1] = h.ny, o.normal[2] = h.nz, o.reserved = h.reserved;
  }
  return RT_OK;
}

// rt_occluded_host (rt.h): the checks, then per ray rq_scan_any
inline int occluded_host_pass(const rt_scene* s, const rt_ray* rays, const int32_t* last, size_t n, uint8_t* out,
                              const char** why) {
  if ((*why = rq_args_error(s, rays, n, out)) != nullptr) return RT_E_ARG;
  std::vector<float> geo;
  rq_tables(*s, &geo, nullptr);
  for (size_t i = 0; i < n; ++i) {
    const rt_ray& q = rays[i];
    FhRay r;
    float tbest;
    out[i] = rq_ray(q.o[0], q.o[1], q.o[2], q.t_min, q.d[0], q.d[1], q.d[2], q.t_max, r, tbest) &&
                     rq_scan_any(r, geo.data(), s->n, tbest, last ? rq_guard(geo.data(), s->n, last[i]) : -1)
                 ? 1
                 : 0;
  }
  return RT_OK;
}

#if defined(__HIPCC__) && defined(RT_RAY_QUERY_KERNEL) && defined(RT_FIRST_HIT_KERNEL)
// ---------------------------------------------------------- the kernels ----
static_assert(sizeof(rt_ray) == 32 && sizeof(rt_ray_hit) == 32, "rt.h: two 16-byte halves each");

struct alignas(16) RqArgs {
  const float4* geo;    // n: cx, cy, cz, -r^2 (the scan)
  const float4* sph;    // n: cx, cy, cz, 1/r (the record's normal)
  const float4* blob;   // the tree (FEAT_LDS, FEAT_GLOBAL)
  int blob_f4, off_pairs, off_pidx, leaf_pairs, big_pair0, n_big_leaves, ref_mul;
  float bvh_c[3], bvh_r, bvh_c0;
  int n;                // bodies
  unsigned n_rays;      // <= 2^31 - 1
  const float4* rays;   // n_rays x 2: (o, t_min), (d, t_max)
  const int32_t* last;  // nullable: n_rays
  float4* hits;         // rays_kernel: n_rays x 2
  uint8_t* occ;         // occluded_kernel: n_rays
};

// ids_kernel's frame at one dimension: 256 threads, a ray a thread.  SRC as
// feat_kernel's; under FEAT_LDS the workgroup stages the tree's image once and
// then takes blocks of 256 rays grid-stride (the host sizes the grid to the
// resident workgroups: a 23 KB image per 256 rays would cost more than the
// rays), the u16 [entry][lane] walk stack behind the image.  Per ray: two
// 16-byte loads, `last`'s 4 bytes (and the 16 bytes of the body it names), and
// (ANY) one byte, or the hit body's two table entries and two 16-byte stores.
template <int SRC, bool ANY>
__device__ __forceinline__ void rq_kernel_body(const RqArgs& a, float4* s_rq_img) {
  const int t = static_cast<int>(threadIdx.x);
  if constexpr (SRC == FEAT_LDS) {
    for (int i = t; i < a.blob_f4; i += kFeatThreads) s_rq_img[i] = a.blob[i];
    __syncthreads();
  }
  FhTree tr;
  tr.base = SRC == FEAT_LDS ? reinterpret_cast<const char*>(s_rq_img) : reinterpret_cast<const char*>(a.blob);
  tr.off_pairs = a.off_pairs, tr.off_pidx = a.off_pidx, tr.leaf_pairs = a.leaf_pairs;
  tr.big_pair0 = a.big_pair0, tr.n_big_leaves = a.n_big_leaves, tr.ref_mul = a.ref_mul;
  tr.c[0] = a.bvh_c[0], tr.c[1] = a.bvh_c[1], tr.c[2] = a.bvh_c[2], tr.r = a.bvh_r, tr.c0 = a.bvh_c0;
  unsigned short* stack0 = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(s_rq_img) +
                                                             (SRC == FEAT_LDS ? a.blob_f4 * 16 : 0));
  const unsigned stride = gridDim.x * static_cast<unsigned>(kFeatThreads);
  // (i < n_rays < 2^31 and stride <= 2^31: the sum stays below 2^32)
  for (unsigned i = blockIdx.x * static_cast<unsigned>(kFeatThreads) + static_cast<unsigned>(t); i < a.n_rays;
       i += stride) {
    const float4 ro = a.rays[2 * static_cast<size_t>(i)], rd = a.rays[2 * static_cast<size_t>(i) + 1];
    const int last = a.last ? rq_guard(reinterpret_cast<const float*>(a.geo), a.n, a.last[i]) : -1;
    FhRay r;
    float tbest;
    const bool active = rq_ray(ro.x, ro.y, ro.z, ro.w, rd.x, rd.y, rd.z, rd.w, r, tbest);
    if constexpr (ANY) {
      bool any = false;
      if (active) {
        if constexpr (SRC == FEAT_SCAN) {
          any = rq_scan_any(r, reinterpret_cast<const float*>(a.geo), a.n, tbest, last);
        } else {
          FhLdsStack stk{stack0 + t, 0};
          any = fh_walk_any<true>(r, tr, stk, tbest, last);
        }
      }
      a.occ[i] = any ? 1 : 0;
    } else {
      RqHit h = rq_none();
      if (active) {
        FhBest best{tbest, -1};
        if constexpr (SRC == FEAT_SCAN) {
          fh_scan<true>(r, reinterpret_cast<const float*>(a.geo), a.n, best, last);
        } else {
          FhLdsStack stk{stack0 + t, 0};
          fh_walk<true>(r, tr, stk, best, last);
        }
        if (best.body >= 0) {
          const float4 sp = a.sph[best.body];
          const float sph4[4] = {sp.x, sp.y, sp.z, sp.w};
          h = rq_record(r, best, rd.x, rd.y, rd.z, sph4, -a.geo[best.body].w);
        }
      }
      float4* o = a.hits + 2 * static_cast<size_t>(i);
      o[0] = make_float4(__int_as_float(h.body), __int_as_float(h.front), h.t, h.dist);
      o[1] = make_float4(h.nx, h.ny, h.nz, h.reserved);
    }
  }
}

template <int SRC>
__global__ __launch_bounds__(kFeatThreads) void rays_kernel(const RqArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 s_rq_img[];   // the tree's blob, then the stack rows
  rq_kernel_body<SRC, false>(a, s_rq_img);
}
template <int SRC>
__global__ __launch_bounds__(kFeatThreads) void occluded_kernel(const RqArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 s_rq_img[];
  rq_kernel_body<SRC, true>(a, s_rq_img);
}
#endif  // __HIPCC__ && RT_RAY_QUERY_KERNEL

}  // namespace rtclj
