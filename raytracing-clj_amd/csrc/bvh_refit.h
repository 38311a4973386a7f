// bvh_refit.h — refitting a scene's trees to bodies that moved
// (rt_scene_update, rt_tree_refit_host; include/rt.h).
//
// Replaces nothing in the reference: its hit-anything (src/raytracing.clj:33-43)
// scans the bodies and has no tree to keep up to date.  The trees are bvh.cpp's;
// every traversal variant returns the scan's hit whatever conservative tree it
// walks, so a refitted tree changes timing only.
//
// Three parts.
//  1. One text for host and device: the outward rounding (nextafter as integer
//     operations on the bits), a body's box, a box relative to the tree centre,
//     "the box of a child from the bodies under it" and the leaf records'
//     centres.  Every bound is one fp32 subtraction or addition (or one fp64
//     subtraction, rounded to fp32 once) followed by the integer step: nothing
//     to contract, no library call, so host and device give the same bytes.
//     Unions are min / max, exact and order-free.  bvh.cpp's build uses the
//     same functions.
//  2. The host: the blob as rt_scene_upload lays it out (tree_pack), the level
//     order a refit walks (tree_levels), the preconditions (refit_spheres_error)
//     and the refit itself (tree_refit), defined in tree_blob.cpp.
//  3. The device kernel (under __HIPCC__ and RT_REFIT_KERNEL): one launch of
//     3 + ceil(n / 1024) workgroups.  Workgroup k < 3 refits tree k: its leaf
//     records first, then its nodes level by level from the deepest, a node's
//     own box (the union of its two child boxes) kept in LDS for its parent,
//     one barrier per level.  The other workgroups rewrite the body tables.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/rt.h"
#include "bvh.h"

#if defined(__HIPCC__)
// (spelt out: bvh.cpp and tree_blob.cpp include this without the HIP runtime header)
#define RT_RF_FN __host__ __device__ inline __attribute__((always_inline))
#define RT_RF_UNROLL _Pragma("unroll")
#else
#define RT_RF_FN inline
#define RT_RF_UNROLL
#endif

namespace rtclj {

// ------------------------------------------------------- the one text ----
RT_RF_FN uint32_t rf_bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
RT_RF_FN float rf_float(uint32_t u) {
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}

// std::nextafter(x, +inf) on the bits: +-0 -> the smallest subnormal, a
// negative value one step towards zero (the smallest negative subnormal ->
// -0), -inf -> -FLT_MAX, FLT_MAX -> +inf; +inf and NaN unchanged
RT_RF_FN float rf_up(float x) {
  const uint32_t u = rf_bits(x), mag = u & 0x7fffffffu;
  if (mag > 0x7f800000u || u == 0x7f800000u) return x;
  if (mag == 0u) return rf_float(1u);
  return rf_float((u >> 31) ? u - 1u : u + 1u);
}
// std::nextafter(x, -inf): the mirror image
RT_RF_FN float rf_down(float x) { return rf_float(rf_bits(rf_up(rf_float(rf_bits(x) ^ 0x80000000u))) ^ 0x80000000u); }

struct RfBox {
  float lo[3], hi[3];
};
RT_RF_FN RfBox rf_none() { return RfBox{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}}; }
// std::min's and std::max's selects
RT_RF_FN float rf_min(float a, float b) { return b < a ? b : a; }
RT_RF_FN float rf_max(float a, float b) { return a < b ? b : a; }
RT_RF_FN void rf_add(RfBox& a, const RfBox& b) {
RT_RF_UNROLL
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = rf_min(a.lo[k], b.lo[k]);
    a.hi[k] = rf_max(a.hi[k], b.hi[k]);
  }
}

// exact float box of a body (cx, cy, cz, r), rounded outward
RT_RF_FN RfBox rf_body_box(const float* s) {
  RfBox b;
  const float r = fabsf(s[3]);
RT_RF_UNROLL
  for (int k = 0; k < 3; ++k) {
    b.lo[k] = rf_down(s[k] - r);
    b.hi[k] = rf_up(s[k] + r);
  }
  return b;
}

// a bound relative to the tree centre: the difference in double, rounded to
// float once.  inf - inf (a bound and the centre both infinite) is NaN: the
// one NaN an x86 host makes of it, on either side.
RT_RF_FN float rf_rel(float bound, float centre) {
  const float v = static_cast<float>(static_cast<double>(bound) - static_cast<double>(centre));
  return v != v ? rf_float(0xffc00000u) : v;
}

// A tree as the refit sees it: the blob nodes | pairs | pidx of bvh.h / bvh.cpp.
struct RfTree {
  char* blob;
  int off_pairs, off_pidx;
  int idx_bytes;    // 4: int indices, -1 a pad; 2: u16, 0xffff a pad
  int leaf_pairs;   // pairs per leaf: 1, 2 or 4
  int n_nodes;
  int n_pairs;      // the tree's leaves' and the big bodies'
  int ref_div;      // an inner-child ref / ref_div = the node's index (80 for the 4-body tree's byte offsets)
  int empty;        // no body in the tree: both root boxes are the point 0
  float c[3];       // the tree centre the stored boxes are relative to
};

// the body of leaf slot `slot` (pair slot / 2, lane slot % 2), -1 for a pad
RT_RF_FN int rf_body(const RfTree& t, int slot) {
  const char* p = t.blob + t.off_pidx;
  if (t.idx_bytes == 2) {
    const uint16_t v = reinterpret_cast<const uint16_t*>(p)[slot];
    return v == 0xffffu ? -1 : static_cast<int>(v);
  }
  return reinterpret_cast<const int*>(p)[slot];
}

// a leaf record's centre: x, y, z of slot's body (w = -r^2, the pads, pidx stay)
RT_RF_FN void rf_slot_centre(const RfTree& t, int slot, const float* sph) {
  const int body = rf_body(t, slot);
  if (body < 0) return;
  float* p = reinterpret_cast<float*>(t.blob + t.off_pairs) + 8 * static_cast<size_t>(slot >> 1) + (slot & 1);
  const float* s = sph + 4 * static_cast<size_t>(body);
  p[0] = s[0];
  p[2] = s[1];
  p[4] = s[2];
}

// the box of the leaf whose first pair is `pair`
RT_RF_FN RfBox rf_leaf_box(const RfTree& t, int pair, const float* sph) {
  RfBox b = rf_none();
  for (int slot = 2 * pair; slot < 2 * (pair + t.leaf_pairs); ++slot) {
    const int body = rf_body(t, slot);
    if (body >= 0) rf_add(b, rf_body_box(sph + 4 * static_cast<size_t>(body)));
  }
  return b;
}

// One node: each child's box from the bodies under it -- a leaf's from its
// bodies, an inner child's as the union its own pass left in `boxes` (Boxes:
// get(node), set(node, box)) -- stored relative to the centre, rounded
// outward, per axis (min, max, min) for the two children (bvh.h); the union of
// the two goes to `boxes` for the parent.  Child refs are read, never written.
template <class Boxes>
RT_RF_FN void rf_node(const RfTree& t, int node, const float* sph, Boxes& boxes) {
  float* w = reinterpret_cast<float*>(t.blob + sizeof(BvhNode) * static_cast<size_t>(node));
  const int* child = reinterpret_cast<const int*>(w + 18);
  RfBox me = rf_none();
  for (int c = 0; c < 2; ++c) {
    const int ref = child[c];
    RfBox b;
    if (t.empty) b = RfBox{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    else if (ref < 0) b = rf_leaf_box(t, ~ref, sph);
    else b = boxes.get(t.ref_div == 1 ? ref : ref / static_cast<int>(sizeof(BvhNode)));
    rf_add(me, b);
RT_RF_UNROLL
    for (int k = 0; k < 3; ++k) {
      const float lo = rf_down(rf_rel(b.lo[k], t.c[k]));
      w[6 * k + c] = lo;
      w[6 * k + 2 + c] = rf_up(rf_rel(b.hi[k], t.c[k]));
      w[6 * k + 4 + c] = lo;
    }
  }
  boxes.set(node, me);
}

// ------------------------------------------------------------- the host ----
// (tree_blob.cpp; each returns RT_OK, or RT_E_ARG with *why set)

// BVH build: surface-area splits (default) or median splits (RTCLJ_BVH=median, for A/B)
bool bvh_sah_default();

// bvh's tree k as rt_scene_upload lays it out: nodes | pairs | pidx padded to
// 16 bytes; the 4-body tree's (k = 1) inner-child refs as byte offsets (bvh's
// own refs are rewritten), the 8-body tree's (k = 2) indices as u16
void tree_pack(BvhHost& bvh, int k, std::vector<char>* blob, rt_tree_info* info);

RfTree tree_view(char* blob, const rt_tree_info& info);
// info and the blob's refs and indices are those of a tree over n bodies
int tree_check(const char* blob, const rt_tree_info& info, int n, const char** why);
// the tree's bodies (those under its nodes: the big bodies' leaves excluded), ascending
std::vector<int> tree_bodies(const char* blob, const rt_tree_info& info);
// The order a refit visits the nodes in: by depth, the deepest level first,
// lvl[l] .. lvl[l + 1] the positions of level l's nodes (a node's inner
// children are all in earlier levels).
void tree_levels(const char* blob, const rt_tree_info& info, std::vector<int>* order, std::vector<int>* lvl);
// rt_scene_update's preconditions on the spheres (rt.h), NULL when they hold
const char* refit_spheres_error(const float* at_upload, const float* now, int n);
// the definition of rt.h applied to a host blob; info's centre and radius updated
int tree_refit(char* blob, rt_tree_info* info, const float* at_upload, const float* now, int n, const char** why);
int tree_cost(const char* blob, const rt_tree_info& info, double* cost, const char** why);

#if defined(__HIPCC__) && defined(RT_REFIT_KERNEL)
// ----------------------------------------------------------- the kernel ----
constexpr int kRefitThreads = 1024;
constexpr int kRefitLevels = kBvhStack;   // (a tree's depth <= kBvhStack - 2, bvh.h)

struct RefitTreeArgs {
  char* blob;
  const int* order;   // tree_levels' order
  int off_pairs, off_pidx, idx_bytes, leaf_pairs, n_nodes, n_pairs, ref_div, empty;
  int n_levels;
  int lvl[kRefitLevels + 1];
  float c[3];
};
struct RefitArgs {
  RefitTreeArgs t[3];
  const float4* src;   // the new spheres (cx, cy, cz, r), n of them
  float4* geo;
  float* geo2;
  float4* sph;
  int n;
};

// the nodes' own boxes in LDS, one plane per bound (no two lanes of a level
// share a node, consecutive nodes fall into consecutive banks)
struct RfLdsBoxes {
  float* p;
  int n;
  __device__ __forceinline__ RfBox get(int node) const {
    RfBox b;
RT_RF_UNROLL
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = p[k * n + node];
      b.hi[k] = p[(3 + k) * n + node];
    }
    return b;
  }
  __device__ __forceinline__ void set(int node, const RfBox& b) {
RT_RF_UNROLL
    for (int k = 0; k < 3; ++k) {
      p[k * n + node] = b.lo[k];
      p[(3 + k) * n + node] = b.hi[k];
    }
  }
};

// Dynamic LDS: 24 bytes x the largest tree's node count.  THREADS: the
// workgroup's size (kRefitThreads).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void refit_kernel(RefitArgs a) {
  extern __shared__ float rf_lds[];
  const int tid = static_cast<int>(threadIdx.x);
  if (blockIdx.x >= 3) {
    // the body tables: geo and its pair-interleaved copy through fh_geo, sph's
    // centre (its 1/r lane stays)
    const int i = (static_cast<int>(blockIdx.x) - 3) * THREADS + tid;
    if (i >= a.n) return;
    const float4 s = a.src[i];
    const float q[4] = {s.x, s.y, s.z, s.w};
    float g[4];
    fh_geo(q, g);
    a.geo[i] = make_float4(g[0], g[1], g[2], g[3]);
    float* o = a.geo2 + 8 * static_cast<size_t>(i >> 1) + (i & 1);
    o[0] = g[0];
    o[2] = g[1];
    o[4] = g[2];
    o[6] = g[3];
    float* p = reinterpret_cast<float*>(a.sph + i);
    p[0] = s.x;
    p[1] = s.y;
    p[2] = s.z;
    return;
  }
  const RefitTreeArgs& ta = a.t[blockIdx.x];
  const RfTree t{ta.blob, ta.off_pairs, ta.off_pidx, ta.idx_bytes, ta.leaf_pairs, ta.n_nodes,
                 ta.n_pairs, ta.ref_div,  ta.empty,    {ta.c[0], ta.c[1], ta.c[2]}};
  const float* sph = reinterpret_cast<const float*>(a.src);
  for (int slot = tid; slot < 2 * t.n_pairs; slot += THREADS) rf_slot_centre(t, slot, sph);
  RfLdsBoxes boxes{rf_lds, t.n_nodes};
  for (int l = 0; l < ta.n_levels; ++l) {
    for (int i = ta.lvl[l] + tid; i < ta.lvl[l + 1]; i += THREADS) rf_node(t, ta.order[i], sph, boxes);
    __syncthreads();
  }
}
#endif  // __HIPCC__ && RT_REFIT_KERNEL

}  // namespace rtclj
