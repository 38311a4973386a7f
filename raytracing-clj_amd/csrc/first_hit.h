// first_hit.h — the first-hit feature pass (rt_launch_feat, include/rt.h):
// albedo, normal, depth and coverage of the first surface a camera ray meets.
//
// Replaces nothing the reference computes on its own: it exposes what its
// per-pixel loop builds and drops --
//   compute-pixel's camera ray          src/raytracing.clj:144-151
//   hit-anything (closest-hit scan)     src/raytracing.clj:33-43
//   sphere ::hit-fn, the hit record     src/hittable.clj:7-31, hit.clj:14-15
//   the materials' ::attenuation        src/material.clj:13-46
//   the sky of a ray that hits nothing  src/raytracing.clj:55-58
//
// Two parts.
//  1. The hit search as plain inline functions that compile for the device
//     (feat_kernel, below) and for the host (tools/first_hit_check.cpp, the
//     CPU test's driver): the ray set-up from (o, d), the body test, the
//     acceptance, the linear scan, and a stack walk over a tree blob
//     (nodes | pairs | pidx, bvh.h / bvh.cpp) that takes the big bodies'
//     leaves first and culls with bvh_pad.h's padded slabs.  One text for
//     both: the fp32 op sequence is trace_kernel.h's (blocks `setup`, the
//     scan, `consider_tie`), without the self-hit guard -- a camera ray
//     leaves no body.  sqrt and 1/x are correctly rounded on either side
//     (fp_rn.h on the device, std::sqrt and IEEE division on the host), so
//     host and device give the same bits.  Beside the walk, its twin for
//     occlusion queries (fh_walk_any: out at the first body, ray_query.h).
//  2. The device kernel (under __HIPCC__): one 256-thread workgroup per 8 x 8
//     tile.  Lane q of each of the four waves owns pixel q of the tile; wave w
//     traces the samples k = w, w + 4, ... of its pixels and keeps their
//     integer sums in registers, the four waves' sums meet in LDS (integer
//     atomics), and the workgroup issues one global atomic per pixel word.
//     The camera sample is trace_kernel.h's block `camera`, op for op, with
//     its RNG helpers (included, not edited).
#pragma once
#include <cmath>
#include <cstdint>

#include "bvh.h"
#include "bvh_pad.h"

#if defined(__HIPCC__)
#include "fp_rn.h"
#define RT_FH_FN __host__ __device__ __forceinline__
#else
#define RT_FH_FN inline
#endif

namespace rtclj {

// ------------------------------------------------------ the hit search ----
// correctly rounded sqrt and reciprocal: the same bits on host and device
RT_FH_FN float fh_sqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}
RT_FH_FN float fh_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return rcp_rn(x);
#else
  return 1.0f / x;
#endif
}

// a ray as the search sees it: origin, unit direction, |d| and t-min
struct FhRay {
  float ox, oy, oz, ux, uy, uz, len, tmin;
};
// trace_kernel.h block `setup`: |d| and 1/|d| correctly rounded,
// u = d * (1/|d|), t-min = 1e-3 in |d| units (raytracing.clj:48)
RT_FH_FN FhRay fh_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
  FhRay r;
  const float len2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  r.len = fh_sqrt(len2);
  const float il = fh_rcp(r.len);
  r.ox = ox, r.oy = oy, r.oz = oz;
  r.ux = dx * il, r.uy = dy * il, r.uz = dz * il;
  r.tmin = 1e-3f * r.len;
  return r;
}

// the closest hit so far: t = +inf, body = -1 before any
struct FhBest {
  float t;
  int body;
};
RT_FH_FN FhBest fh_none() { return FhBest{INFINITY, -1}; }

// One body (centre, -r^2) of index s: the scan's oc, h, c, disc, the nearer
// root, else the farther one (hittable.clj:15-18), accepted iff t > t-min and
// (t, s) is lexicographically smaller than the best (raytracing.clj:35-42's
// strict compare in array order).  The pre-test is the scan's candidate test,
// min(disc, max(h, -c)) >= 0: what it drops has no root above t-min.  A root
// of +inf (a body whose r * r overflows) is no hit: t < best.t fails against
// "none yet" and -1 is below every index.
// GUARD (spec_chain.h): the body the ray is leaving, `last`, takes sq = |h| for
// sqrt(disc), trace_kernel.h's self-hit guard (`consider`); without it, the
// default, `last` is not read and the code is what it was.
template <bool GUARD = false>
RT_FH_FN void fh_test(const FhRay& r, float cx, float cy, float cz, float nr2, int s, FhBest& b, int last = -1) {
  const float ocx = cx - r.ox, ocy = cy - r.oy, ocz = cz - r.oz;
  const float h = fmaf(r.uz, ocz, fmaf(r.uy, ocy, r.ux * ocx));
  const float c = fmaf(ocx, ocx, fmaf(ocz, ocz, fmaf(ocy, ocy, nr2)));
  const float disc = fmaf(h, h, -c);
  if (!(fminf(disc, fmaxf(h, -c)) >= 0.0f)) return;
  float sq;
  if constexpr (GUARD) sq = s == last ? fabsf(h) : fh_sqrt(disc);
  else sq = fh_sqrt(disc);
  const float tn = h - sq;
  const float t = tn > r.tmin ? tn : h + sq;
  const bool acc = (t > r.tmin) & ((t < b.t) | ((t == b.t) & (s < b.body)));
  b.t = acc ? t : b.t;
  b.body = acc ? s : b.body;
}

// A body's entry in the scan's table from its (cx, cy, cz, r): the centre and
// -r^2, the square rounded once.  The one construction: rt_scene_upload's
// table and rt_ids_host's are both made here.
RT_FH_FN void fh_geo(const float* sphere4, float* geo4) {
  const float r = sphere4[3];
  geo4[0] = sphere4[0], geo4[1] = sphere4[1], geo4[2] = sphere4[2];
  geo4[3] = -(r * r);
}

// the linear scan: geo = n x (cx, cy, cz, -r^2), in array order
template <bool GUARD = false>
RT_FH_FN void fh_scan(const FhRay& r, const float* geo, int n, FhBest& b, int last = -1) {
  for (int s = 0; s < n; ++s) fh_test<GUARD>(r, geo[4 * s], geo[4 * s + 1], geo[4 * s + 2], geo[4 * s + 3], s, b, last);
}

// A tree as the walk reads it: `base` = the blob nodes | pairs | pidx
// (BvhNode of bvh.h, 80 bytes; pairs of 8 floats x0 x1 y0 y1 z0 z1 w0 w1; two
// int indices per pair).  ref_mul: what turns an inner-child ref into the
// node's byte offset (80 for bvh_build's node indices, 1 for the 4-body
// tree's device copy, whose refs rt_scene_upload multiplied already).
struct FhTree {
  const char* base;
  int off_pairs, off_pidx;
  int leaf_pairs;              // pairs per leaf: 1, 2 or 4
  int big_pair0, n_big_leaves;
  int ref_mul;
  float c[3], r, c0;           // bounding sphere, kPadRmax x r_max (bvh_pad.h)
};

// a leaf: its pairs' bodies, each by fh_test (a pad has -r^2 = +inf: disc = -inf)
template <bool GUARD = false>
RT_FH_FN void fh_leaf(const FhRay& r, const FhTree& t, int p, FhBest& b, int last = -1) {
  const float* g = reinterpret_cast<const float*>(t.base + t.off_pairs) + 8 * static_cast<size_t>(p);
  const int* id = reinterpret_cast<const int*>(t.base + t.off_pidx) + 2 * static_cast<size_t>(p);
  for (int q = 0; q < t.leaf_pairs; ++q, g += 8, id += 2) {
    fh_test<GUARD>(r, g[0], g[2], g[4], g[6], id[0], b, last);
    fh_test<GUARD>(r, g[1], g[3], g[5], g[7], id[1], b, last);
  }
}

// The walk.  Stack: push(unsigned) / pop(unsigned&) -> bool of node byte
// offsets, at most depth - 1 entries at a time (one pending far child per
// level above the current node).  Every body the scan would accept lies in
// every padded box on its path (bvh_pad.h), a box is skipped only if its
// padded interval misses (t-min, best], and the acceptance is the scan's in
// any order: the result is fh_scan's, bit for bit.
template <bool GUARD = false, class Stack>
RT_FH_FN void fh_walk(const FhRay& r, const FhTree& t, Stack& st, FhBest& b, int last = -1) {
  // 1) the big bodies, kept out of the tree (bvh.cpp): their hits cull the tree
  for (int k = 0; k < t.n_big_leaves; ++k) fh_leaf<GUARD>(r, t, t.big_pair0 + k * t.leaf_pairs, b, last);
  // 2) the tree, nearer child first
  const float ex = r.ox - t.c[0], ey = r.oy - t.c[1], ez = r.oz - t.c[2];
  const PadRay pr = pad_ray(ex, ey, ez, r.ux, r.uy, r.uz, t.r, t.c0);
  const PadAxis ax = pad_axis(r.ux, ex, r.tmin, pr), ay = pad_axis(r.uy, ey, r.tmin, pr),
                az = pad_axis(r.uz, ez, r.tmin, pr);
  // byte offsets of an axis' (near, far) plane pairs inside a node: + 8 for u < 0
  const unsigned offx = ax.sign >> 28, offy = 24u + (ay.sign >> 28), offz = 48u + (az.sign >> 28);
  unsigned node = 0;
  for (;;) {
    const char* nb = t.base + node;
    const float* px = reinterpret_cast<const float*>(nb + offx);   // near (c0, c1), far (c0, c1)
    const float* py = reinterpret_cast<const float*>(nb + offy);
    const float* pz = reinterpret_cast<const float*>(nb + offz);
    const int c0 = reinterpret_cast<const int*>(nb + 72)[0], c1 = reinterpret_cast<const int*>(nb + 72)[1];
    float tn0, tf0, tn1, tf1;
    pad_interval(ax, ay, az, px[0], px[2], py[0], py[2], pz[0], pz[2], tn0, tf0);
    pad_interval(ax, ay, az, px[1], px[3], py[1], py[3], pz[1], pz[3], tn1, tf1);
    const bool hit0 = pad_meets(tn0, tf0, r.tmin, b.t), hit1 = pad_meets(tn1, tf1, r.tmin, b.t);
    if (hit0 && c0 < 0) fh_leaf<GUARD>(r, t, ~c0, b, last);
    if (hit1 && c1 < 0) fh_leaf<GUARD>(r, t, ~c1, b, last);
    const bool i0 = hit0 && c0 >= 0, i1 = hit1 && c1 >= 0;
    const unsigned n0 = static_cast<unsigned>(c0) * static_cast<unsigned>(t.ref_mul),
                   n1 = static_cast<unsigned>(c1) * static_cast<unsigned>(t.ref_mul);
    if (i0 && i1) {
      const bool sw = tn1 < tn0;
      st.push(sw ? n0 : n1);
      node = sw ? n1 : n0;
    } else if (i0 || i1) {
      node = i0 ? n0 : n1;
    } else if (!st.pop(node)) {
      break;
    }
  }
}

// The walk of an occlusion query (ray_query.h): is any body met in
// (t-min, tmax)?  fh_walk's big-body leaves first and its padded-box cull,
// against the fixed interval (t-min, tmax] -- nothing is "closest" here, so the
// children are taken in tree order, no near/far compare, and the walk returns
// at the first leaf that accepted a body.  Until then the best stays
// {tmax, -1}, so every body meets fh_test's acceptance against that pair: the
// predicate is "fh_scan from {tmax, -1} ends on a body", body for body.
template <bool GUARD = false, class Stack>
RT_FH_FN bool fh_walk_any(const FhRay& r, const FhTree& t, Stack& st, float tmax, int last = -1) {
  FhBest b{tmax, -1};
  for (int k = 0; k < t.n_big_leaves; ++k) {
    fh_leaf<GUARD>(r, t, t.big_pair0 + k * t.leaf_pairs, b, last);
    if (b.body >= 0) return true;
  }
  const float ex = r.ox - t.c[0], ey = r.oy - t.c[1], ez = r.oz - t.c[2];
  const PadRay pr = pad_ray(ex, ey, ez, r.ux, r.uy, r.uz, t.r, t.c0);
  const PadAxis ax = pad_axis(r.ux, ex, r.tmin, pr), ay = pad_axis(r.uy, ey, r.tmin, pr),
                az = pad_axis(r.uz, ez, r.tmin, pr);
  const unsigned offx = ax.sign >> 28, offy = 24u + (ay.sign >> 28), offz = 48u + (az.sign >> 28);
  unsigned node = 0;
  for (;;) {
    const char* nb = t.base + node;
    const float* px = reinterpret_cast<const float*>(nb + offx);
    const float* py = reinterpret_cast<const float*>(nb + offy);
    const float* pz = reinterpret_cast<const float*>(nb + offz);
    const int c0 = reinterpret_cast<const int*>(nb + 72)[0], c1 = reinterpret_cast<const int*>(nb + 72)[1];
    float tn0, tf0, tn1, tf1;
    pad_interval(ax, ay, az, px[0], px[2], py[0], py[2], pz[0], pz[2], tn0, tf0);
    pad_interval(ax, ay, az, px[1], px[3], py[1], py[3], pz[1], pz[3], tn1, tf1);
    const bool hit0 = pad_meets(tn0, tf0, r.tmin, tmax), hit1 = pad_meets(tn1, tf1, r.tmin, tmax);
    if (hit0 && c0 < 0) fh_leaf<GUARD>(r, t, ~c0, b, last);
    if (hit1 && c1 < 0) fh_leaf<GUARD>(r, t, ~c1, b, last);
    if (b.body >= 0) return true;
    const bool i0 = hit0 && c0 >= 0, i1 = hit1 && c1 >= 0;
    const unsigned n0 = static_cast<unsigned>(c0) * static_cast<unsigned>(t.ref_mul),
                   n1 = static_cast<unsigned>(c1) * static_cast<unsigned>(t.ref_mul);
    if (i0 && i1) {
      st.push(n1);
      node = n0;
    } else if (i0 || i1) {
      node = i0 ? n0 : n1;
    } else if (!st.pop(node)) {
      return false;
    }
  }
}

// Resolve of one pixel (rt_feat_resolve, rt_feat_resolve_host): the six sums
// (albedo rgb as unsigned, normal xyz as signed 2^-24 units), the hit count,
// the nearest distance and nf = RN(float(max(samples, 1))) -> 8 floats, each
// step one IEEE fp32 operation (rt_launch's conversion, with the division).
RT_FH_FN void fh_resolve(const long long* sums, unsigned hits, float depth, float nf, float* out) {
  for (int c = 0; c < 3; ++c)
    out[c] = static_cast<float>(static_cast<unsigned long long>(sums[c])) * 0x1p-24f / nf;
  for (int c = 3; c < 6; ++c) out[c] = static_cast<float>(sums[c]) * 0x1p-24f / nf;
  out[6] = depth;
  out[7] = static_cast<float>(hits) / nf;
}

}  // namespace rtclj

// ---------------------------------------------------------- the kernel ----
// (for the unit that launches it: first_hit.hip defines RT_FIRST_HIT_KERNEL
// before it includes this file)
#if defined(__HIPCC__) && defined(RT_FIRST_HIT_KERNEL)
#include "trace_kernel.h"

namespace rtclj {

enum { FEAT_LDS = 0, FEAT_GLOBAL = 1, FEAT_SCAN = 2 };   // where the bodies come from
constexpr int kFeatThreads = 256;

struct alignas(16) FeatArgs {
  const float4* geo;    // n_pad: cx, cy, cz, -r^2 (the scan)
  const float4* sph;    // n: cx, cy, cz, 1/r
  const float4* mat;    // n: albedo rgb, ...
  const int* kind;      // n
  const float4* blob;   // the tree (FEAT_LDS, FEAT_GLOBAL)
  int blob_f4, off_pairs, off_pidx, leaf_pairs, big_pair0, n_big_leaves, ref_mul;
  float bvh_c[3], bvh_r, bvh_c0;
  float cam[18];        // center, p00, du, dv, disk_u, disk_v
  int defocus, sampler;
  int n;
  int width, rows_out, row_begin, row_tile, tile_first, tile_step, tiles_x;
  int spp, sample_begin;
  uint32_t key;
  unsigned long long* sums;       // rows_out x width x 6 (two's complement)
  unsigned* hits;                 // rows_out x width
  unsigned* depth;                // rows_out x width, float bits
  unsigned long long* counters;   // nullable: += {segments, samples}
};

// the lane's walk stack: u16 entries (node byte offset / 16: below 2^16 for
// RT_MAX_SPHERES bodies), [entry][lane] in LDS (no bank conflicts, no scratch)
struct FhLdsStack {
  unsigned short* slot;   // the lane's entry 0
  int n;
  __device__ __forceinline__ void push(unsigned node) {
    slot[n * kFeatThreads] = static_cast<unsigned short>(node >> 4);
    ++n;
  }
  __device__ __forceinline__ bool pop(unsigned& node) {
    if (n == 0) return false;
    --n;
    node = static_cast<unsigned>(slot[n * kFeatThreads]) << 4;
    return true;
  }
};

// n * 2^24 toward zero as i32 (v_cvt_i32_f32: NaN gives 0; |n| stays far below 2^7)
__device__ __forceinline__ int fix24s(float c) {
  int r;
  asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(c * 0x1p24f));
  return r;
}

template <int SRC>
__global__ __launch_bounds__(kFeatThreads) void feat_kernel(const FeatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 s_img[];   // the tree's blob, then the stack rows
  __shared__ unsigned long long s_sum[kPoolPx * 6];
  __shared__ unsigned s_hits[kPoolPx], s_depth[kPoolPx];
  const int t = static_cast<int>(threadIdx.x);
  if constexpr (SRC == FEAT_LDS)
    for (int i = t; i < a.blob_f4; i += kFeatThreads) s_img[i] = a.blob[i];
  for (int i = t; i < kPoolPx * 6; i += kFeatThreads) s_sum[i] = 0ull;
  if (t < kPoolPx) {
    s_hits[t] = 0u;
    s_depth[t] = 0x7f800000u;
  }
  __syncthreads();
  // the workgroup's tile; lane q of every wave owns pool pixel q
  const int tile = static_cast<int>(blockIdx.x);
  const int tby = tile / a.tiles_x, tbx = tile - tby * a.tiles_x;
  const int q = t & (kPoolPx - 1), wave = t >> 6;
  const int px = tbx * kTile + (q & (kTile - 1)), ro = tby * kTile + (q >> 3);
  const bool inside = px < a.width && ro < a.rows_out;
  if (inside && wave < a.spp) {
    // compacted output row -> image row (interleaved row tiles), the pixel's RNG key
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
    unsigned long long sr = 0, sg = 0, sb = 0;
    long long nx = 0, ny = 0, nz = 0;
    unsigned hits = 0, dmin = 0x7f800000u;
    for (int k = wave; k < a.spp; k += kFeatThreads / 64) {
      // ---- compute-pixel, one sample (raytracing.clj:144-151; trace_kernel.h `camera`) ----
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
      const float dx = sx - ox, dy = sy - oy, dz = sz - oz;
      // ---- hit-anything (raytracing.clj:33-43) ----
      const FhRay r = fh_ray(ox, oy, oz, dx, dy, dz);
      FhBest best = fh_none();
      if constexpr (SRC == FEAT_SCAN) {
        fh_scan(r, reinterpret_cast<const float*>(a.geo), a.n, best);
      } else {
        FhLdsStack stk{stack0 + t, 0};
        fh_walk(r, tr, stk, best);
      }
      if (best.body < 0) {
        // the sky (raytracing.clj:55-58), trace_kernel.h's ops
        const float sa = 0.5f * (r.uy + 1.0f);
        const float om = 1.0f - sa;
        sr += fix24(fmaf(sa, 0.5f, om));
        sg += fix24(fmaf(sa, 0.7f, om));
        sb += fix24(fmaf(sa, 1.0f, om));
      } else {
        // the hit record (hittable.clj:24-31, hit.clj:14-15; trace_kernel.h `hit`)
        const float4 sp = a.sph[best.body];
        const float hx = fmaf(r.ux, best.t, ox), hy = fmaf(r.uy, best.t, oy), hz = fmaf(r.uz, best.t, oz);
        float ux = (hx - sp.x) * sp.w, uy = (hy - sp.y) * sp.w, uz = (hz - sp.z) * sp.w;
        const bool front = fmaf(dz, uz, fmaf(dy, uy, dx * ux)) < 0.0f;
        if (!front) {
          ux = -ux;
          uy = -uy;
          uz = -uz;
        }
        // Block `hit`'s normal is only as long as the fp32 root lies on the
        // surface: P is off it by about d(disc) / (2 r), so |n| is off by
        // d(disc) / (2 r^2) -- 1e-3 for an r = 0.2 body 13 units away.  A
        // guide wants a unit vector: scaled here by one correctly rounded
        // 1 / |n| (sqrt and reciprocal as in `setup`; (0, 0, 1) stays exact;
        // a zero or NaN n becomes NaN, which the conversion turns into 0).
        const float nil = fh_rcp(fh_sqrt(fmaf(uz, uz, fmaf(uy, uy, ux * ux))));
        ux = ux * nil;
        uy = uy * nil;
        uz = uz * nil;
        nx += fix24s(ux);
        ny += fix24s(uy);
        nz += fix24s(uz);
        // ::attenuation (material.clj:13-46): the albedo; glass attenuates by 1; no material, black
        const int kind = a.kind[best.body];
        if (kind == RT_LAMBERTIAN || kind == RT_METAL) {
          const float4 m = a.mat[best.body];
          sr += fix24(m.x);
          sg += fix24(m.y);
          sb += fix24(m.z);
        } else if (kind == RT_DIELECTRIC) {
          sr += 1ull << 24;
          sg += 1ull << 24;
          sb += 1ull << 24;
        }
        ++hits;
        dmin = min(dmin, __float_as_uint(best.t));   // t > 0: the bits order like the floats
      }
    }
    // the four waves' sums of a pixel meet in LDS (integers: any order)
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
  }
  __syncthreads();
  // One global atomic per pixel word and workgroup; a pixel outside the frame
  // is never touched.  The sums: a tile row's 8 pixels x 6 words are 48
  // consecutive u64 in LDS (word i of the tile: row i / 48) and in the frame,
  // so thread i brings word i -- a wave's lanes cover whole 64-byte lines
  // where a wave bringing one word of every pixel touched six times as many
  // (384 words: threads 0 .. 255, then 0 .. 127 again).  The hit counts and
  // the depths go with waves 2 and 3, a lane per pixel.
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
    const unsigned long long traced = static_cast<unsigned long long>(vw * vh) * static_cast<unsigned long long>(a.spp);
    atomicAdd(&a.counters[0], traced);   // one segment per sample
    atomicAdd(&a.counters[1], traced);
  }
}

// rt_feat_add: another rt_feat's contents (staged in HBM) merged into this
// one's by the atomics a pass uses -- sums and hit counts added, the depth by
// minimum -- so that a pass on another stream may touch the same words
__global__ __launch_bounds__(256) void feat_add_kernel(unsigned long long* __restrict__ sums, unsigned* __restrict__ hits,
                                                        unsigned* __restrict__ depth,
                                                        const unsigned long long* __restrict__ add_sums,
                                                        const unsigned* __restrict__ add_hits,
                                                        const unsigned* __restrict__ add_depth, size_t n_px) {
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n_px; i += stride) {
    for (int c = 0; c < 6; ++c) {
      const unsigned long long v = add_sums[i * 6 + c];
      if (v) __hip_atomic_fetch_add(&sums[i * 6 + c], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned h = add_hits[i], d = add_depth[i];
    if (h) __hip_atomic_fetch_add(&hits[i], h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (d < 0x7f800000u) __hip_atomic_fetch_min(&depth[i], d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// rt_feat_resolve: a thread per pixel, fh_resolve's conversion; the buffers are only read
__global__ __launch_bounds__(256) void feat_resolve_kernel(const unsigned long long* __restrict__ sums,
                                                            const unsigned* __restrict__ hits,
                                                            const unsigned* __restrict__ depth, size_t n_px, float nf,
                                                            float* __restrict__ out) {
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n_px; i += stride) {
    long long s[6];
    for (int c = 0; c < 6; ++c) s[c] = static_cast<long long>(sums[i * 6 + c]);
    float o[8];
    fh_resolve(s, hits[i], __uint_as_float(depth[i]), nf, o);
    for (int c = 0; c < 8; ++c) out[i * 8 + c] = o[c];
  }
}

}  // namespace rtclj
#endif  // __HIPCC__ && RT_FIRST_HIT_KERNEL
