// refit.hip — a scene's trees refitted on the device for moved bodies:
// rt_scene_update and refit_kernel (bvh_refit.h), and the read-outs of a
// scene's trees (rt_scene_tree_info, rt_scene_tree_read).  DESIGN.md §3.11.
#include "trace_kernel.h"
#include "first_hit.h"
#define RT_REFIT_KERNEL
#include "bvh_refit.h"
#include "dscene.h"

using namespace rtclj;

static rt_tree_info tree_info_of(const rt_dscene& ds, int k) {
  const DTree& t = ds.tree[k];
  rt_tree_info ti{};
  ti.n_nodes = t.n_nodes;
  ti.off_pairs = t.off_pairs;
  ti.off_pidx = t.off_pidx;
  ti.blob_bytes = t.blob_f4 * 16;
  ti.big_pair0 = t.big_pair0;
  ti.n_big_leaves = t.n_big_leaves;
  ti.depth = t.depth;
  ti.leaf_size = 2 << k;
  ti.idx_bytes = k == 2 ? 2 : 4;
  for (int j = 0; j < 3; ++j) ti.center[j] = t.c[j];
  ti.radius = t.r;
  ti.c0 = t.c0;
  return ti;
}

extern "C" int rt_scene_tree_info(const rt_dscene* ds, int k, rt_tree_info* info) {
  clear_error();
  if (!ds || !info) return set_error(RT_E_ARG, "rt_scene_tree_info: NULL argument");
  if (k < 0 || k > 2) return set_error(RT_E_ARG, "rt_scene_tree_info: k must be 0, 1 or 2");
  *info = tree_info_of(*ds, k);
  return RT_OK;
}

extern "C" int rt_scene_tree_read(const rt_dscene* ds, int k, void* blob, size_t cap, void* hip_stream) {
  clear_error();
  const std::string me("rt_scene_tree_read");
  if (!ds || !blob) return set_error(RT_E_ARG, me + ": NULL argument");
  if (k < 0 || k > 2) return set_error(RT_E_ARG, me + ": k must be 0, 1 or 2");
  const size_t bytes = static_cast<size_t>(ds->tree[k].blob_f4) * 16;
  if (cap < bytes) return set_error(RT_E_ARG, me + ": the blob needs " + std::to_string(bytes) + " bytes");
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device(me, stream, ds->device, "the scene")) return rc;
  HIP_TRY(hipSetDevice(ds->device));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(blob, ds->tree[k].blob, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

// the first update's allocations: the spheres' device copy, the level orders,
// the staging ring
static int refit_prepare(rt_dscene& d) {
  RefitState& rf = d.refit;
  if (rf.ready) return RT_OK;
  hipError_t e = rf.src.alloc(static_cast<size_t>(d.n));
  std::vector<int> all;
  for (int k = 0; k < 3; ++k) all.insert(all.end(), rf.order[k].begin(), rf.order[k].end());
  if (e == hipSuccess) e = rf.d_order.alloc(all.size());
  if (e == hipSuccess) e = hipMemcpy(rf.d_order.p, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice);
  for (int i = 0; i < kRefitSlots && e == hipSuccess; ++i) {
    e = hipHostMalloc(reinterpret_cast<void**>(&rf.pin[i]), 4 * sizeof(float) * static_cast<size_t>(d.n), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&rf.ev[i], hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    rf.release();
    return hip_fail(e, "rt_scene_update");
  }
  rf.ready = true;
  return RT_OK;
}

extern "C" int rt_scene_update(rt_dscene* ds, const float* sphere, void* hip_stream) {
  clear_error();
  const std::string me("rt_scene_update");
  if (!ds || (!sphere && ds->n > 0)) return set_error(RT_E_ARG, me + ": NULL argument");
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device(me, stream, ds->device, "the scene")) return rc;
  RefitState& rf = ds->refit;
  std::lock_guard<std::mutex> lk(rf.mu);
  const int n = ds->n;
  if (const char* why = refit_spheres_error(rf.sph0.data(), sphere, n)) return set_error(RT_E_ARG, me + ": " + why);
  if (n == 0) return RT_OK;   // (no body: no table entry, and the trees' boxes are the point 0)
  // the launch arguments of the trees: one body set, so one centre and radius
  float c[3], r = 0.0f, r_max = 0.0f;
  bvh_bounds(sphere, rf.bodies.data(), static_cast<int>(rf.bodies.size()), c, &r, &r_max);
  HIP_TRY(hipSetDevice(ds->device));
  if (const int rc = refit_prepare(*ds)) return rc;
  RefitArgs a{};
  size_t max_nodes = 1, at = 0;
  for (int k = 0; k < 3; ++k) {
    const DTree& t = ds->tree[k];
    RefitTreeArgs& ta = a.t[k];
    const int n_levels = static_cast<int>(rf.lvl[k].size()) - 1;
    if (n_levels > kRefitLevels) return set_error(RT_E_ARG, me + ": a tree is deeper than the build allows");
    ta.blob = reinterpret_cast<char*>(t.blob);
    ta.order = rf.d_order.p + at;
    at += rf.order[k].size();
    ta.off_pairs = t.off_pairs;
    ta.off_pidx = t.off_pidx;
    ta.idx_bytes = k == 2 ? 2 : 4;
    ta.leaf_pairs = 1 << k;
    ta.n_nodes = t.n_nodes;
    ta.n_pairs = (t.off_pidx - t.off_pairs) / 32;
    ta.ref_div = k == 1 ? static_cast<int>(sizeof(BvhNode)) : 1;
    ta.empty = rf.empty;
    ta.n_levels = n_levels;
    for (int l = 0; l <= n_levels; ++l) ta.lvl[l] = rf.lvl[k][l];
    for (int j = 0; j < 3; ++j) ta.c[j] = c[j];
    max_nodes = std::max(max_nodes, static_cast<size_t>(t.n_nodes));
  }
  a.src = rf.src.p;
  a.geo = ds->geo;
  a.geo2 = reinterpret_cast<float*>(ds->geo2);
  a.sph = ds->sph;
  a.n = n;
  const size_t lds = 6 * sizeof(float) * max_nodes;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&refit_kernel<kRefitThreads>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(lds)));
  // the caller's array into a staging slot whose last copy has run, then
  // stream-ordered: the copy to the device, the kernel
  const int slot = rf.next;
  HIP_TRY(hipEventSynchronize(rf.ev[slot]));
  const size_t bytes = 4 * sizeof(float) * static_cast<size_t>(n);
  std::memcpy(rf.pin[slot], sphere, bytes);
  HIP_TRY(hipMemcpyAsync(rf.src.p, rf.pin[slot], bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(rf.ev[slot], stream));
  rf.next = (slot + 1) % kRefitSlots;
  const unsigned blocks = 3u + static_cast<unsigned>((n + kRefitThreads - 1) / kRefitThreads);
  HIP_TRY(enqueue(refit_kernel<kRefitThreads>, dim3(blocks), dim3(kRefitThreads), lds, stream, a));
  for (int k = 0; k < 3; ++k) {
    for (int j = 0; j < 3; ++j) ds->tree[k].c[j] = c[j];
    ds->tree[k].r = r;
  }
  return RT_OK;
}
