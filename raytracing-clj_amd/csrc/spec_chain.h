// spec_chain.h — the specular-chain feature pass (rt_launch_feat_chain,
// rt_feat_chain_host, include/rt.h): the guides of what glass and mirrors
// show.  A camera ray is followed through the deterministic part of its path
// -- mirror reflections (metal of fuzz <= fuzz_max, drawn as fuzz 0) and the
// dielectric's refraction branch -- to the first rough surface or the sky, and
// the features are taken there: albedo times the chain's throughput, the
// world-space normal of the last surface, the path length so far.
//
// Replaces nothing the reference computes on its own: it exposes what
// ray-color's recursion passes through and drops --
//   ray-color, one level                 src/raytracing.clj:45-58
//   hit-anything (closest-hit scan)      src/raytracing.clj:33-43
//   sphere ::hit-fn, the hit record      src/hittable.clj:7-31, hit.clj:14-15
//   metal ::scatter-fn (reflect)         src/material.clj:21-28
//   dielectric ::scatter-fn              src/realm/raytracing.clj:158-177
//   the materials' ::attenuation         src/material.clj:13-46
//   the sky of a ray that hits nothing   src/raytracing.clj:55-58
//
// Three parts, as first_hit.h and body_ids.h.
//  1. One segment as plain inline functions that compile for the device
//     (chain_kernel, below) and for the host (rt_feat_chain_host,
//     tools/chain_check.cpp): first_hit.h's search with the self-hit guard
//     switched on (no text of its own for the body test, the acceptance or the
//     walk), then sc_surface -- the hit record, the smoothness test, the
//     metal's and the dielectric's new direction, the end of the chain.  The
//     fp32 op sequences are trace_kernel.h's blocks `hit`, `lambert_metal`
//     (the metal half, without its draw) and `dielectric` (as under
//     RT_FLAG_REALM), op for op.
//  2. The pass on the host, checks included (chain_host_pass): what
//     rt_feat_chain_host runs, and what tools/chain_check.cpp runs under the
//     sanitizers.
//  3. The device kernel (under __HIPCC__ and RT_SPEC_CHAIN_KERNEL, after
//     first_hit.h's kernel part): feat_kernel's frame around one segment loop.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/rt.h"
#include "first_hit.h"

namespace rtclj {

// ---------------------------------------------------------- one segment ----
// a sample's chain between two segments
struct ScState {
  float ox, oy, oz, dx, dy, dz;   // the ray, d un-normalised
  float tr, tg, tb;               // throughput: the product of the mirrors' albedos
  float L;                        // the length of the segments behind
  int last, b;                    // the body the ray leaves (-1: the camera), bounces taken
};
RT_FH_FN ScState sc_start(float ox, float oy, float oz, float dx, float dy, float dz) {
  return ScState{ox, oy, oz, dx, dy, dz, 1.0f, 1.0f, 1.0f, 0.0f, -1, 0};
}
// where a chain ended: the floats before their conversion to 2^-24 units
struct ScEnd {
  int body;   // -1: the sky
  float ar, ag, ab, nx, ny, nz;
};

// The body tables as rt_scene_upload lays them out for the kernels: sph4 =
// (cx, cy, cz, 1/r), mat4 = the material floats, a dielectric's lane 0 = 1/eta
// (the ri of a front face) and lane 3 = eta.  IEEE divisions, the same bits.
inline void sc_tables(const rt_scene& s, float* sph4, float* mat4) {
  for (int i = 0; i < s.n; ++i) {
    const float* q = s.sphere + 4 * static_cast<size_t>(i);
    const float* m = s.mat + 4 * static_cast<size_t>(i);
    float *sp = sph4 + 4 * static_cast<size_t>(i), *mt = mat4 + 4 * static_cast<size_t>(i);
    sp[0] = q[0], sp[1] = q[1], sp[2] = q[2], sp[3] = 1.0f / q[3];
    mt[0] = m[0], mt[1] = m[1], mt[2] = m[2], mt[3] = m[3];
    if (s.mat_kind[i] == RT_DIELECTRIC) mt[0] = 1.0f / m[3];
  }
}

// What the closest hit `best` of the segment r = fh_ray(s.o, s.d) means for the
// chain.  true: the body is smooth and a bounce is left -- s holds the next
// segment.  false: the chain ended, on the sky or on this surface -- e holds
// its features and s.L the depth (unchanged on a miss).
// sph, mat: 4 floats per body (sc_tables' layout), 16-byte aligned on the device.
RT_FH_FN bool sc_surface(ScState& s, const FhRay& r, const FhBest& best, const float* sph, const float* mat,
                         const int* kind, int max_bounces, float fuzz_max, ScEnd& e) {
  if (best.body < 0) {
    // the sky (raytracing.clj:55-58), trace_kernel.h's ops
    const float sa = 0.5f * (r.uy + 1.0f);
    const float om = 1.0f - sa;
    e.body = -1;
    e.ar = s.tr * fmaf(sa, 0.5f, om);
    e.ag = s.tg * fmaf(sa, 0.7f, om);
    e.ab = s.tb * fmaf(sa, 1.0f, om);
    e.nx = e.ny = e.nz = 0.0f;
    return false;
  }
  s.L = s.L + best.t;
  // the hit record (hittable.clj:24-31, hit.clj:14-15; trace_kernel.h `hit`)
  const float* sp = sph + 4 * static_cast<size_t>(best.body);
  const float* m = mat + 4 * static_cast<size_t>(best.body);
  const float hx = fmaf(r.ux, best.t, s.ox), hy = fmaf(r.uy, best.t, s.oy), hz = fmaf(r.uz, best.t, s.oz);
  float nx = (hx - sp[0]) * sp[3], ny = (hy - sp[1]) * sp[3], nz = (hz - sp[2]) * sp[3];
  const bool front = fmaf(s.dz, nz, fmaf(s.dy, ny, s.dx * nx)) < 0.0f;
  if (!front) {
    nx = -nx;
    ny = -ny;
    nz = -nz;
  }
  const int k = kind[best.body];
  const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
  const bool smooth = k == RT_DIELECTRIC || (k == RT_METAL && m3 <= fuzz_max);   // (a NaN fuzz is rough)
  if (smooth && s.b < max_bounces) {
    bool on = true;
    if (k == RT_METAL) {
      // material.clj:21-28 with fuzz 0: reflect the un-normalised d; no draw
      const float k2 = 2.0f * fmaf(s.dz, nz, fmaf(s.dy, ny, s.dx * nx));
      const float rx = fmaf(-nx, k2, s.dx), ry = fmaf(-ny, k2, s.dy), rz = fmaf(-nz, k2, s.dz);
      on = fmaf(rz, nz, fmaf(ry, ny, rx * nx)) > 0.0f;
      if (on) {
        s.dx = rx, s.dy = ry, s.dz = rz;
        s.tr *= m0;
        s.tg *= m1;
        s.tb *= m2;
      }
    } else {
      // realm/raytracing.clj:158-177: no Schlick term, no draw
      const float ri = front ? m0 : m3;   // 1/eta : eta
      const float un = fmaf(r.uz, nz, fmaf(r.uy, ny, r.ux * nx));
      const float cosv = fminf(-un, 1.0f);
      const float sinv = fh_sqrt(fmaf(-cosv, cosv, 1.0f));
      if (!(ri * sinv <= 1.0f)) {
        const float k2 = 2.0f * un;
        s.dx = fmaf(-nx, k2, r.ux);
        s.dy = fmaf(-ny, k2, r.uy);
        s.dz = fmaf(-nz, k2, r.uz);
      } else {
        const float qx = fmaf(nx, cosv, r.ux) * ri;
        const float qy = fmaf(ny, cosv, r.uy) * ri;
        const float qz = fmaf(nz, cosv, r.uz) * ri;
        const float par = -fh_sqrt(fabsf(1.0f - fmaf(qz, qz, fmaf(qy, qy, qx * qx))));
        s.dx = fmaf(nx, par, qx);
        s.dy = fmaf(ny, par, qy);
        s.dz = fmaf(nz, par, qz);
      }
    }
    if (on) {
      s.ox = hx, s.oy = hy, s.oz = hz;
      s.last = best.body;
      ++s.b;
      return true;
    }
  }
  // the chain ends on this surface: ::attenuation (material.clj:13-46) under
  // the throughput, and feat_kernel's unit normal (one correctly rounded 1/|n|)
  const float a0 = k == RT_DIELECTRIC ? 1.0f : k == RT_NONE ? 0.0f : m0;
  const float a1 = k == RT_DIELECTRIC ? 1.0f : k == RT_NONE ? 0.0f : m1;
  const float a2 = k == RT_DIELECTRIC ? 1.0f : k == RT_NONE ? 0.0f : m2;
  e.body = best.body;
  e.ar = s.tr * a0;
  e.ag = s.tg * a1;
  e.ab = s.tb * a2;
  const float nil = fh_rcp(fh_sqrt(fmaf(nz, nz, fmaf(ny, ny, nx * nx))));
  e.nx = nx * nil;
  e.ny = ny * nil;
  e.nz = nz * nil;
  return false;
}

// ------------------------------------------------------------- the host ----
// rt_feat_chain_opts' defaults and checks: nullptr, or why not
inline const char* chain_opts_resolve(const rt_feat_chain_opts* o, rt_feat_chain_opts* out) {
  out->max_bounces = 8;
  out->fuzz_max = 0.0f;
  if (!o) return nullptr;
  if (o->max_bounces < 0 || o->max_bounces > 64) return "max_bounces outside 0..64";
  if (!(o->fuzz_max >= 0.0f) || !std::isfinite(o->fuzz_max)) return "fuzz_max is not finite and >= 0";
  *out = *o;
  return nullptr;
}

// rt_feat_chain_host (rt.h): the checks, then per ray the segment loop over
// fh_scan's linear scan (guarded).  0, or an error code with *why set.
inline int chain_host_pass(const rt_scene* s, const rt_feat_chain_opts* opts, const float* rays, size_t n,
                           rt_chain_sample* out, const char** why) {
  *why = nullptr;
  if (!s || (n > 0 && (!rays || !out))) {
    *why = "NULL argument";
    return RT_E_ARG;
  }
  if (s->n < 0 || (s->n > 0 && (!s->sphere || !s->mat_kind || !s->mat))) {
    *why = "bad scene arrays";
    return RT_E_ARG;
  }
  for (int i = 0; i < s->n; ++i) {
    const int k = s->mat_kind[i];
    if (k != RT_LAMBERTIAN && k != RT_METAL && k != RT_DIELECTRIC && k != RT_NONE) {
      *why = "unsupported material kind";
      return RT_E_MATERIAL;
    }
  }
  rt_feat_chain_opts o;
  if ((*why = chain_opts_resolve(opts, &o)) != nullptr) return RT_E_ARG;
  const size_t nb = static_cast<size_t>(s->n);
  std::vector<float> geo(4 * nb), sph(4 * nb), mat(4 * nb);
  for (size_t b = 0; b < nb; ++b) fh_geo(s->sphere + 4 * b, &geo[4 * b]);
  sc_tables(*s, sph.data(), mat.data());
  for (size_t i = 0; i < n; ++i) {
    const float* q = rays + 6 * i;
    ScState st = sc_start(q[0], q[1], q[2], q[3], q[4], q[5]);
    ScEnd e;
    for (;;) {
      const FhRay r = fh_ray(st.ox, st.oy, st.oz, st.dx, st.dy, st.dz);
      FhBest best = fh_none();
      fh_scan<true>(r, geo.data(), s->n, best, st.last);
      if (!sc_surface(st, r, best, sph.data(), mat.data(), s->mat_kind, o.max_bounces, o.fuzz_max, e)) break;
    }
    rt_chain_sample& c = out[i];
    c.body = e.body;
    c.bounces = st.b;
    c.length = e.body < 0 ? INFINITY : st.L;
    c.albedo[0] = e.ar, c.albedo[1] = e.ag, c.albedo[2] = e.ab;
    c.normal[0] = e.nx, c.normal[1] = e.ny, c.normal[2] = e.nz;
  }
  return RT_OK;
}

}  // namespace rtclj

// ---------------------------------------------------------- the kernel ----
#if defined(__HIPCC__) && defined(RT_SPEC_CHAIN_KERNEL) && defined(RT_FIRST_HIT_KERNEL)
namespace rtclj {

struct alignas(16) ChainArgs {
  FeatArgs f;
  int max_bounces;
  float fuzz_max;
};

// feat_kernel's frame -- one 256-thread workgroup per 8 x 8 tile, lane q of each
// wave owns pixel q, wave w the samples w, w + 4, ..., sums in registers, met in
// LDS by integer atomics, one global atomic per pixel word, the u16
// [entry][lane] walk stack -- around one segment loop: a lane holds a sample's
// chain (ScState) and its sample index k; every iteration traces one segment
// through the one walk call site, and a lane whose chain ends there adds the
// sample to its sums and takes its next one at the head of the next iteration,
// while its neighbours go on bouncing.  The wave leaves the loop when every
// lane has run out of samples.
template <int SRC>
__global__ __launch_bounds__(kFeatThreads) void chain_kernel(const ChainArgs ca) {
  const FeatArgs& a = ca.f;
  extern __shared__ __attribute__((aligned(16))) float4 s_img[];   // the tree's blob, then the stack rows
  __shared__ unsigned long long s_sum[kPoolPx * 6];
  __shared__ unsigned s_hits[kPoolPx], s_depth[kPoolPx];
  __shared__ unsigned long long s_segs;
  const int t = static_cast<int>(threadIdx.x);
  if constexpr (SRC == FEAT_LDS)
    for (int i = t; i < a.blob_f4; i += kFeatThreads) s_img[i] = a.blob[i];
  for (int i = t; i < kPoolPx * 6; i += kFeatThreads) s_sum[i] = 0ull;
  if (t < kPoolPx) {
    s_hits[t] = 0u;
    s_depth[t] = 0x7f800000u;
  }
  if (t == 0) s_segs = 0ull;
  __syncthreads();
  const int tile = static_cast<int>(blockIdx.x);
  const int tby = tile / a.tiles_x, tbx = tile - tby * a.tiles_x;
  const int q = t & (kPoolPx - 1), wave = t >> 6;
  const int px = tbx * kTile + (q & (kTile - 1)), ro = tby * kTile + (q >> 3);
  const bool inside = px < a.width && ro < a.rows_out;
  if (inside && wave < a.spp) {
    int gy = a.row_begin + ro;
    if (a.tile_step > 0) {
      const int rt = ro / a.row_tile;
      gy = a.row_begin + (a.tile_first + rt * a.tile_step) * a.row_tile + (ro - rt * a.row_tile);
    }
    const uint32_t pk =
        mix32(a.key ^ mix32(static_cast<uint32_t>(gy) * static_cast<uint32_t>(a.width) + static_cast<uint32_t>(px)));
    const float fpx = static_cast<float>(px), fgy = static_cast<float>(gy);
    FhTree tr;
    tr.base = SRC == FEAT_LDS ? reinterpret_cast<const char*>(s_img) : reinterpret_cast<const char*>(a.blob);
    tr.off_pairs = a.off_pairs, tr.off_pidx = a.off_pidx, tr.leaf_pairs = a.leaf_pairs;
    tr.big_pair0 = a.big_pair0, tr.n_big_leaves = a.n_big_leaves, tr.ref_mul = a.ref_mul;
    tr.c[0] = a.bvh_c[0], tr.c[1] = a.bvh_c[1], tr.c[2] = a.bvh_c[2], tr.r = a.bvh_r, tr.c0 = a.bvh_c0;
    unsigned short* stack0 = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(s_img) +
                                                               (SRC == FEAT_LDS ? a.blob_f4 * 16 : 0));
    const float* sph = reinterpret_cast<const float*>(__builtin_assume_aligned(a.sph, 16));
    const float* mat = reinterpret_cast<const float*>(__builtin_assume_aligned(a.mat, 16));
    unsigned long long sr = 0, sg = 0, sb = 0;
    long long nx = 0, ny = 0, nz = 0;
    unsigned hits = 0, dmin = 0x7f800000u, segs = 0;
    ScState s{};
    int k = wave;
    bool fresh = true;
    for (;;) {
      if (fresh) {
        if (k >= a.spp) break;
        // ---- compute-pixel, one sample: feat_kernel's block, op for op ----
        uint32_t st = mix32(pk + static_cast<uint32_t>(a.sample_begin + k) * 0x9e3779b9u);
        if (st == 0) st = 0x6d2b79f5u;
        const float fx = fpx + rng_centered(st);
        const float fy = fgy + rng_centered(st);
        const float sx = fmaf(a.cam[9], fy, fmaf(a.cam[6], fx, a.cam[3]));
        const float sy = fmaf(a.cam[10], fy, fmaf(a.cam[7], fx, a.cam[4]));
        const float sz = fmaf(a.cam[11], fy, fmaf(a.cam[8], fx, a.cam[5]));
        float ox = a.cam[0], oy = a.cam[1], oz = a.cam[2];
        if (a.defocus) {
          float qx, qy;
          if (a.sampler & RT_SAMPLER_DISK) {
            disk_direct(st, qx, qy);
          } else {
            do {
              qx = rng_sym(st);
              qy = rng_sym(st);
            } while (!(fmaf(qy, qy, qx * qx) < 1.0f));
          }
          ox = fmaf(a.cam[15], qy, fmaf(a.cam[12], qx, a.cam[0]));
          oy = fmaf(a.cam[16], qy, fmaf(a.cam[13], qx, a.cam[1]));
          oz = fmaf(a.cam[17], qy, fmaf(a.cam[14], qx, a.cam[2]));
        }
        s = sc_start(ox, oy, oz, sx - ox, sy - oy, sz - oz);
        fresh = false;
      }
      // ---- one segment: hit-anything (raytracing.clj:33-43), guarded ----
      const FhRay r = fh_ray(s.ox, s.oy, s.oz, s.dx, s.dy, s.dz);
      FhBest best = fh_none();
      if constexpr (SRC == FEAT_SCAN) {
        fh_scan<true>(r, reinterpret_cast<const float*>(a.geo), a.n, best, s.last);
      } else {
        FhLdsStack stk{stack0 + t, 0};
        fh_walk<true>(r, tr, stk, best, s.last);
      }
      ++segs;
      ScEnd e;
      if (!sc_surface(s, r, best, sph, mat, a.kind, ca.max_bounces, ca.fuzz_max, e)) {
        sr += fix24(e.ar);
        sg += fix24(e.ag);
        sb += fix24(e.ab);
        if (e.body >= 0) {
          nx += fix24s(e.nx);
          ny += fix24s(e.ny);
          nz += fix24s(e.nz);
          ++hits;
          dmin = min(dmin, __float_as_uint(s.L));   // L > 0: the bits order like the floats
        }
        k += kFeatThreads / 64;
        fresh = true;
      }
    }
    unsigned long long* ps = s_sum + q * 6;
    if (sr) atomicAdd(ps + 0, sr);
    if (sg) atomicAdd(ps + 1, sg);
    if (sb) atomicAdd(ps + 2, sb);
    if (nx) atomicAdd(ps + 3, static_cast<unsigned long long>(nx));
    if (ny) atomicAdd(ps + 4, static_cast<unsigned long long>(ny));
    if (nz) atomicAdd(ps + 5, static_cast<unsigned long long>(nz));
    if (hits) {
      atomicAdd(&s_hits[q], hits);
      atomicMin(&s_depth[q], dmin);
    }
    if (a.counters) atomicAdd(&s_segs, static_cast<unsigned long long>(segs));
  }
  __syncthreads();
  // feat_kernel's write-out: one global atomic per pixel word and workgroup
  if (a.spp > 0) {
    const int px0 = tbx * kTile, ro0 = tby * kTile;
    for (int i = t; i < kPoolPx * 6; i += kFeatThreads) {
      const int row = i / (kTile * 6), off = i - row * (kTile * 6);
      const unsigned long long v = s_sum[i];
      if (v && ro0 + row < a.rows_out && px0 + off / 6 < a.width)
        __hip_atomic_fetch_add(&a.sums[(static_cast<size_t>(ro0 + row) * a.width + px0) * 6 + off], v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    if (inside && wave >= 2) {
      const size_t e = static_cast<size_t>(ro) * a.width + px;
      if (wave == 2) {
        const unsigned v = s_hits[q];
        if (v) __hip_atomic_fetch_add(&a.hits[e], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        const unsigned v = s_depth[q];
        if (v != 0x7f800000u) __hip_atomic_fetch_min(&a.depth[e], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (a.counters && t == 0 && a.spp > 0) {
    const int vw = max(0, min(kTile, a.width - tbx * kTile)), vh = max(0, min(kTile, a.rows_out - tby * kTile));
    atomicAdd(&a.counters[0], s_segs);
    atomicAdd(&a.counters[1], static_cast<unsigned long long>(vw * vh) * static_cast<unsigned long long>(a.spp));
  }
}

}  // namespace rtclj
#endif  // __HIPCC__ && RT_SPEC_CHAIN_KERNEL && RT_FIRST_HIT_KERNEL
