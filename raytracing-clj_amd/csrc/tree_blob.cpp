// tree_blob.cpp — a scene's trees as bytes, on the host (plain C++, no device):
// the blob rt_scene_upload uploads for each of bvh.cpp's three trees, and the
// host side of a refit (bvh_refit.h): its preconditions, the
// level order its node pass follows, the pass itself over bvh_refit.h's one
// text, and the surface-area cost that tells how far a refitted tree has
// loosened.  Behind rt_tree_build_host, rt_tree_refit_host, rt_tree_cost_host
// (rt_host.cpp) and rt_scene_upload / rt_scene_update (trace.hip, refit.hip).
#if defined(__HIP__)
#include <hip/hip_runtime.h>   // (the library builds every source as HIP; bvh_pad.h then wants its qualifiers)
#endif

#include "bvh_refit.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "bvh_pad.h"

namespace rtclj {

bool bvh_sah_default() {
  static const bool sah = [] {
    const char* e = std::getenv("RTCLJ_BVH");
    return !(e && std::strcmp(e, "median") == 0);
  }();
  return sah;
}

void tree_pack(BvhHost& bvh, int k, std::vector<char>* blob, rt_tree_info* info) {
  const size_t nb = bvh.nodes.size() * sizeof(BvhNode);
  const size_t pb = bvh.pairs.size() * sizeof(float);
  // body indices: u16 for the 8-body-leaf tree (RT_MAX_SPHERES < 65535; a
  // pad's -1 -> 0xffff, never a candidate), int for the others
  const size_t isz = k == 2 ? sizeof(uint16_t) : sizeof(int);
  std::vector<uint16_t> pidx16(bvh.pidx.size());
  for (size_t i = 0; i < pidx16.size(); ++i) pidx16[i] = static_cast<uint16_t>(bvh.pidx[i]);
  const size_t ib = ((bvh.pidx.size() * isz + 15) / 16) * 16;
  blob->assign(nb + pb + ib, 0);
  if (k == 1)   // 4-body tree: inner-child refs as byte offsets (< 65536 while it fits LDS: u16 stack)
    for (BvhNode& nd : bvh.nodes)
      for (int& c : nd.child)
        if (c >= 0) c *= static_cast<int>(sizeof(BvhNode));
  std::memcpy(blob->data(), bvh.nodes.data(), nb);
  std::memcpy(blob->data() + nb, bvh.pairs.data(), pb);
  if (k == 2) std::memcpy(blob->data() + nb + pb, pidx16.data(), pidx16.size() * sizeof(uint16_t));
  else std::memcpy(blob->data() + nb + pb, bvh.pidx.data(), bvh.pidx.size() * sizeof(int));
  *info = rt_tree_info{};
  info->n_nodes = static_cast<int>(bvh.nodes.size());
  info->off_pairs = static_cast<int>(nb);
  info->off_pidx = static_cast<int>(nb + pb);
  info->blob_bytes = static_cast<int>(blob->size());
  info->big_pair0 = bvh.big_pair0;
  info->n_big_leaves = bvh.n_big_leaves;
  info->depth = bvh.depth;
  info->leaf_size = bvh.leaf_size;
  info->idx_bytes = static_cast<int>(isz);
  for (int j = 0; j < 3; ++j) info->center[j] = bvh.center[j];
  info->radius = bvh.radius;
  info->c0 = kPadRmax * bvh.r_max;
}

static int pairs_of(const rt_tree_info& info) { return (info.off_pidx - info.off_pairs) / 32; }
static int ref_div_of(const rt_tree_info& info) { return info.leaf_size == 4 ? static_cast<int>(sizeof(BvhNode)) : 1; }

RfTree tree_view(char* blob, const rt_tree_info& info) {
  RfTree t{};
  t.blob = blob;
  t.off_pairs = info.off_pairs;
  t.off_pidx = info.off_pidx;
  t.idx_bytes = info.idx_bytes;
  t.leaf_pairs = info.leaf_size / 2;
  t.n_nodes = info.n_nodes;
  t.n_pairs = pairs_of(info);
  t.ref_div = ref_div_of(info);
  t.empty = 1;
  for (int slot = 0; slot < 2 * info.big_pair0 && t.empty; ++slot) t.empty = rf_body(t, slot) < 0;
  for (int j = 0; j < 3; ++j) t.c[j] = info.center[j];
  return t;
}

int tree_check(const char* blob, const rt_tree_info& info, int n, const char** why) {
  *why = "info does not describe a tree";
  if (!blob || n < 0 || n > RT_MAX_SPHERES) return RT_E_ARG;
  if (info.leaf_size != 2 && info.leaf_size != 4 && info.leaf_size != 8) return RT_E_ARG;
  if (info.idx_bytes != (info.leaf_size == 8 ? 2 : 4)) return RT_E_ARG;
  if (info.n_nodes < 1 || info.n_nodes > 2 * RT_MAX_SPHERES || info.depth < 1 || info.depth > kBvhStack) return RT_E_ARG;
  if (info.off_pairs != info.n_nodes * static_cast<int>(sizeof(BvhNode))) return RT_E_ARG;
  if (info.off_pidx < info.off_pairs || (info.off_pidx - info.off_pairs) % 32 != 0) return RT_E_ARG;
  const int n_pairs = pairs_of(info), lp = info.leaf_size / 2;
  if (n_pairs > 2 * RT_MAX_SPHERES + 16) return RT_E_ARG;
  if (info.blob_bytes != info.off_pidx + (2 * n_pairs * info.idx_bytes + 15) / 16 * 16) return RT_E_ARG;
  if (info.big_pair0 < 0 || info.n_big_leaves < 0 || info.big_pair0 + info.n_big_leaves * lp != n_pairs) return RT_E_ARG;
  const RfTree t = tree_view(const_cast<char*>(blob), info);
  *why = "the blob's refs or indices are not those of a tree over n bodies";
  for (int slot = 0; slot < 2 * n_pairs; ++slot) {
    const int b = rf_body(t, slot);
    if (b < -1 || b >= n) return RT_E_ARG;
  }
  for (int i = 0; i < info.n_nodes; ++i) {
    const BvhNode* nd = reinterpret_cast<const BvhNode*>(blob) + i;
    for (int c = 0; c < 2; ++c) {
      const int ref = nd->child[c];
      if (ref < 0) {
        if (~ref > info.big_pair0 - lp || ~ref % lp != 0) return RT_E_ARG;
      } else if (ref % t.ref_div != 0 || ref / t.ref_div <= i || ref / t.ref_div >= info.n_nodes) {
        return RT_E_ARG;   // (the builder numbers a node before its children)
      }
    }
  }
  *why = nullptr;
  return RT_OK;
}

std::vector<int> tree_bodies(const char* blob, const rt_tree_info& info) {
  const RfTree t = tree_view(const_cast<char*>(blob), info);
  std::vector<int> v;
  for (int slot = 0; slot < 2 * info.big_pair0; ++slot) {
    const int b = rf_body(t, slot);
    if (b >= 0) v.push_back(b);
  }
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

void tree_levels(const char* blob, const rt_tree_info& info, std::vector<int>* order, std::vector<int>* lvl) {
  const int n = info.n_nodes, div = ref_div_of(info);
  // a node's index is above its parent's (the builder numbers a node before
  // its children; tree_check): one ascending pass gives every depth
  std::vector<int> depth(n, 0);
  int deepest = 0;
  for (int i = 0; i < n; ++i) {
    const BvhNode* nd = reinterpret_cast<const BvhNode*>(blob) + i;
    for (int c = 0; c < 2; ++c)
      if (nd->child[c] >= 0) {
        depth[nd->child[c] / div] = depth[i] + 1;
        deepest = std::max(deepest, depth[i] + 1);
      }
  }
  lvl->assign(deepest + 2, 0);
  for (int i = 0; i < n; ++i) ++(*lvl)[deepest - depth[i] + 1];
  for (int l = 0; l <= deepest; ++l) (*lvl)[l + 1] += (*lvl)[l];
  order->assign(n, 0);
  std::vector<int> at(lvl->begin(), lvl->end() - 1);
  for (int i = 0; i < n; ++i) (*order)[at[deepest - depth[i]]++] = i;
}

const char* refit_spheres_error(const float* at_upload, const float* now, int n) {
  for (int i = 0; i < n; ++i) {
    const float *a = at_upload + 4 * static_cast<size_t>(i), *b = now + 4 * static_cast<size_t>(i);
    if (std::memcmp(a + 3, b + 3, sizeof(float)) != 0) return "a radius differs from the upload's";
    const float r = a[3];
    if (!std::isfinite(r * r)) continue;   // (left out for its radius: any centre)
    const bool fa = std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]);
    const bool fb = std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2]);
    if (fa != fb) return fa ? "a body of the tree has a centre that is not finite" : "a body left out for its centre has a finite one";
  }
  return nullptr;
}

namespace {
struct HostBoxes {
  std::vector<RfBox> v;
  RfBox get(int node) const { return v[node]; }
  void set(int node, const RfBox& b) { v[node] = b; }
};
}  // namespace

int tree_refit(char* blob, rt_tree_info* info, const float* at_upload, const float* now, int n, const char** why) {
  *why = "NULL argument";
  if (!blob || !info || n < 0 || (n > 0 && (!at_upload || !now))) return RT_E_ARG;
  if (const int rc = tree_check(blob, *info, n, why)) return rc;
  if ((*why = refit_spheres_error(at_upload, now, n)) != nullptr) return RT_E_ARG;
  const std::vector<int> bodies = tree_bodies(blob, *info);
  float r_max = 0.0f;
  bvh_bounds(now, bodies.data(), static_cast<int>(bodies.size()), info->center, &info->radius, &r_max);
  const RfTree t = tree_view(blob, *info);
  for (int slot = 0; slot < 2 * t.n_pairs; ++slot) rf_slot_centre(t, slot, now);
  std::vector<int> order, lvl;
  tree_levels(blob, *info, &order, &lvl);
  HostBoxes boxes{std::vector<RfBox>(t.n_nodes, rf_none())};
  for (int i : order) rf_node(t, i, now, boxes);
  return RT_OK;
}

int tree_cost(const char* blob, const rt_tree_info& info, double* cost, const char** why) {
  *why = "info does not describe a tree";
  if (info.n_nodes < 1 || info.n_nodes > 2 * RT_MAX_SPHERES || info.off_pairs != info.n_nodes * static_cast<int>(sizeof(BvhNode)))
    return RT_E_ARG;
  double sum = 0.0;
  for (int i = 0; i < info.n_nodes; ++i) {
    const BvhNode* nd = reinterpret_cast<const BvhNode*>(blob) + i;
    for (int c = 0; c < 2; ++c) {
      const double dx = double(nd->x[2 + c]) - nd->x[c], dy = double(nd->y[2 + c]) - nd->y[c], dz = double(nd->z[2 + c]) - nd->z[c];
      sum += 2.0 * (dx * dy + dy * dz + dz * dx);
    }
  }
  *cost = sum;
  *why = nullptr;
  return RT_OK;
}

}  // namespace rtclj
