// first_hit.hip — the passes that stop at a camera ray's first hit: the feature
// buffers (rt_feat, rt_launch_feat; first_hit.h's feat_kernel) and the body-id
// pass (rt_launch_ids; body_ids.h's ids_kernel), with their occupancy entries;
// the ray queries (rt_launch_rays, rt_launch_occluded; ray_query.h's kernels);
// and the pass into the same buffers that goes on through mirrors and glass
// (rt_launch_feat_chain; spec_chain.h's chain_kernel).  All follow the trace
// unit's selector (dscene.h).  DESIGN.md §3.7, §3.10, §3.15.
#include "trace_kernel.h"
#define RT_FIRST_HIT_KERNEL
#include "first_hit.h"
#define RT_BODY_IDS_KERNEL
#include "body_ids.h"
#define RT_RAY_QUERY_KERNEL
#include "ray_query.h"
#define RT_SPEC_CHAIN_KERNEL
#include "spec_chain.h"
#include "dscene.h"

using namespace rtclj;

// the policy's copies of the feature kernels' shapes
static_assert(policy::kFeatThreads == kFeatThreads && static_cast<int>(policy::FEAT_LDS) == FEAT_LDS &&
                  static_cast<int>(policy::FEAT_GLOBAL) == FEAT_GLOBAL && static_cast<int>(policy::FEAT_SCAN) == FEAT_SCAN,
              "variant_policy.h: the kernels' shapes");

// ---- first-hit features: albedo, normal, depth, coverage (rt.h, first_hit.h) ----
// Per pixel six 64-bit sums (albedo rgb, normal xyz, 2^-24 units), a u32 hit
// count and the nearest hit distance as float bits, on the scene's device; the
// samples per pixel they hold on the host side, as rt_accum keeps them.
struct rt_feat : FrameBuf {
  size_t n_px = 0;                   // rows_out x width
  DevBuf<unsigned long long> sums;   // n_px x 6
  DevBuf<unsigned> hits;             // n_px
  DevBuf<unsigned> depth;            // n_px, float bits (+inf: no hit yet)
  // the kind of pass held since the last clear (rt_launch_feat_chain, rt.h)
  enum { NONE = 0, FIRST_HIT = 1, CHAIN = 2 };
  int kind = NONE;
  rt_feat_chain_opts chain{};        // kind == CHAIN: its options
};

// the feature kernel for a source of bodies (policy::feat_source)
static const void* feat_fn(int src) {
  return src == FEAT_LDS      ? reinterpret_cast<const void*>(&feat_kernel<FEAT_LDS>)
         : src == FEAT_GLOBAL ? reinterpret_cast<const void*>(&feat_kernel<FEAT_GLOBAL>)
                              : reinterpret_cast<const void*>(&feat_kernel<FEAT_SCAN>);
}

static FeatArgs feat_args(const rt_dscene& dsr, const rt_camera& cr, const rt_params& pr, const rt_feat& fr, int rows,
                          uint64_t* d_counters);

static hipError_t feat_reset(rt_feat* f, hipStream_t stream) {
  hipError_t e = fill_zero(f->sums, f->n_px * 6, stream);
  if (e == hipSuccess) e = fill_zero(f->hits, f->n_px, stream);
  if (e == hipSuccess) e = fill_words(f->depth.p, 0x7f800000u, f->n_px, stream);
  return e;
}

extern "C" int rt_feat_create(const rt_dscene* ds, const rt_params* shape, rt_feat** out) {
  clear_error();
  if (!ds || !shape || !out) return set_error(RT_E_ARG, "rt_feat_create: NULL argument");
  *out = nullptr;
  int rows = 0;
  if (const int rc = frame_rows("rt_feat_create", *shape, &rows)) return rc;
  rt_feat* f = nullptr;
  if (const int rc = frame_new(*ds, *shape, &f)) return rc;
  f->n_px = static_cast<size_t>(rows) * shape->width;
  hipError_t e = f->sums.alloc(f->n_px * 6);
  if (e == hipSuccess) e = f->hits.alloc(f->n_px);
  if (e == hipSuccess) e = f->depth.alloc(f->n_px);
  if (e == hipSuccess) e = feat_reset(f, nullptr);
  return frame_created("rt_feat_create", f, e, out);
}

extern "C" int rt_feat_free(rt_feat* f) { return frame_free(f); }

extern "C" int rt_feat_clear(rt_feat* f, void* hip_stream) {
  clear_error();
  if (!f) return set_error(RT_E_ARG, "rt_feat_clear: NULL argument");
  std::lock_guard<std::mutex> lk(f->mu);
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(feat_reset(f, static_cast<hipStream_t>(hip_stream)));
  f->samples = 0;
  f->kind = rt_feat::NONE;
  return RT_OK;
}

extern "C" int64_t rt_feat_samples(const rt_feat* f) { return frame_samples(f); }

extern "C" int rt_launch_feat(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_feat* f,
                              uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!ds || !c || !p || !f) return set_error(RT_E_ARG, "rt_launch_feat: NULL argument");
  if (const int rc = check_frame_args("rt_launch_feat", *p)) return rc;
  std::lock_guard<std::mutex> lk(f->mu);
  if (const int rc = check_pass("rt_launch_feat", "the feature buffers", *f, *ds, *p)) return rc;
  if (f->kind == rt_feat::CHAIN)
    return set_error(RT_E_ARG, "rt_launch_feat: the feature buffers hold chain passes (rt_feat_clear first)");
  if (p->spp == 0) return RT_OK;
  const int rows = rows_out(*p);
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::feat_source(si, selected_variant(), diag_build());
  FeatArgs a = feat_args(*ds, *c, *p, *f, rows, d_counters);
  const int gy = (rows + kTile - 1) / kTile;
  HIP_TRY(enqueue(feat_fn(src), dim3(static_cast<unsigned>(a.tiles_x * gy)), dim3(kFeatThreads), policy::feat_lds(si, src),
                  static_cast<hipStream_t>(hip_stream), a));
  f->samples += p->spp;
  f->kind = rt_feat::FIRST_HIT;
  return RT_OK;
}

// ---- specular-chain features (rt.h, spec_chain.h) ------------------------------
static const void* chain_fn(int src) {
  return src == FEAT_LDS      ? reinterpret_cast<const void*>(&chain_kernel<FEAT_LDS>)
         : src == FEAT_GLOBAL ? reinterpret_cast<const void*>(&chain_kernel<FEAT_GLOBAL>)
                              : reinterpret_cast<const void*>(&chain_kernel<FEAT_SCAN>);
}

extern "C" int rt_launch_feat_chain(const rt_dscene* ds, const rt_camera* c, const rt_params* p,
                                    const rt_feat_chain_opts* opts, rt_feat* f, uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!ds || !c || !p || !f) return set_error(RT_E_ARG, "rt_launch_feat_chain: NULL argument");
  if (const int rc = check_frame_args("rt_launch_feat_chain", *p)) return rc;
  rt_feat_chain_opts o;
  if (const char* why = chain_opts_resolve(opts, &o)) return set_error(RT_E_ARG, std::string("rt_launch_feat_chain: ") + why);
  std::lock_guard<std::mutex> lk(f->mu);
  if (const int rc = check_pass("rt_launch_feat_chain", "the feature buffers", *f, *ds, *p)) return rc;
  if (f->kind == rt_feat::FIRST_HIT)
    return set_error(RT_E_ARG, "rt_launch_feat_chain: the feature buffers hold first-hit passes (rt_feat_clear first)");
  if (f->kind == rt_feat::CHAIN && (f->chain.max_bounces != o.max_bounces || f->chain.fuzz_max != o.fuzz_max))
    return set_error(RT_E_ARG, "rt_launch_feat_chain: the feature buffers hold chain passes of other options");
  if (p->spp == 0) return RT_OK;
  const int rows = rows_out(*p);
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::feat_source(si, selected_variant(), diag_build());
  ChainArgs a{};
  a.f = feat_args(*ds, *c, *p, *f, rows, d_counters);
  a.max_bounces = o.max_bounces;
  a.fuzz_max = o.fuzz_max;
  const int gy = (rows + kTile - 1) / kTile;
  HIP_TRY(enqueue(chain_fn(src), dim3(static_cast<unsigned>(a.f.tiles_x * gy)), dim3(kFeatThreads),
                  policy::feat_lds(si, src), static_cast<hipStream_t>(hip_stream), a));
  f->samples += p->spp;
  f->kind = rt_feat::CHAIN;
  f->chain = o;
  return RT_OK;
}

// The chain kernel a launch on ds would run under the current selector
// (diagnostic, tools/chain_time.py): out4 as rt_feat_occupancy's.
extern "C" int rt_feat_chain_occupancy(const rt_dscene* ds, int* out4) {
  clear_error();
  if (!ds || !out4) return set_error(RT_E_ARG, "rt_feat_chain_occupancy: NULL argument");
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::feat_source(si, selected_variant(), diag_build());
  if (const int rc = occupancy_report(chain_fn(src), kFeatThreads, policy::feat_lds(si, src), out4)) return rc;
  out4[3] = src;
  return RT_OK;
}

// a pass's kernel arguments (feat_kernel's, and chain_kernel's first part)
static FeatArgs feat_args(const rt_dscene& dsr, const rt_camera& cr, const rt_params& pr, const rt_feat& fr, int rows,
                          uint64_t* d_counters) {
  const rt_dscene* ds = &dsr;
  const rt_camera* c = &cr;
  const rt_params* p = &pr;
  const rt_feat* f = &fr;
  const DTree& tr = ds->tree[1];
  FeatArgs a{};
  a.geo = ds->geo;
  a.sph = ds->sph;
  a.mat = ds->mat;
  a.kind = ds->kind;
  a.blob = tr.blob;
  a.blob_f4 = tr.blob_f4;
  a.off_pairs = tr.off_pairs;
  a.off_pidx = tr.off_pidx;
  a.leaf_pairs = 2;
  a.big_pair0 = tr.big_pair0;
  a.n_big_leaves = tr.n_big_leaves;
  a.ref_mul = 1;   // (rt_scene_upload made the 4-body tree's inner refs byte offsets)
  for (int k = 0; k < 3; ++k) a.bvh_c[k] = tr.c[k];
  a.bvh_r = tr.r;
  a.bvh_c0 = tr.c0;
  pack_frame(a, *c, *p, rows);
  a.n = ds->n;
  a.tiles_x = (p->width + kTile - 1) / kTile;
  a.sums = f->sums.p;
  a.hits = f->hits.p;
  a.depth = f->depth.p;
  a.counters = reinterpret_cast<unsigned long long*>(d_counters);
  return a;
}

extern "C" int rt_feat_resolve(const rt_feat* f, float* d_out, void* hip_stream) {
  clear_error();
  if (!f || !d_out) return set_error(RT_E_ARG, "rt_feat_resolve: NULL argument");
  const int64_t count = frame_samples(f);
  HIP_TRY(hipSetDevice(f->device));
  const float nf = static_cast<float>(count > 0 ? count : 1);   // RN(float(n))
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((f->n_px + 255) / 256, 4096));
  HIP_TRY(enqueue(feat_resolve_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
                  f->sums.p, f->hits.p, f->depth.p, f->n_px, nf, d_out));
  return RT_OK;
}

extern "C" int rt_feat_read(const rt_feat* f, int64_t* host_sums, uint32_t* host_hits, float* host_depth,
                            void* hip_stream) {
  clear_error();
  if (!f || !host_sums || !host_hits || !host_depth) return set_error(RT_E_ARG, "rt_feat_read: NULL argument");
  HIP_TRY(hipSetDevice(f->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_sums, f->sums.p, f->n_px * 6 * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(host_hits, f->hits.p, f->n_px * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(host_depth, f->depth.p, f->n_px * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_feat_add(rt_feat* f, const int64_t* host_sums, const uint32_t* host_hits, const float* host_depth,
                           int64_t samples, void* hip_stream) {
  clear_error();
  if (!f || !host_sums || !host_hits || !host_depth) return set_error(RT_E_ARG, "rt_feat_add: NULL argument");
  std::lock_guard<std::mutex> lk(f->mu);
  if (const int rc = check_add("rt_feat_add", *f, samples)) return rc;
  for (size_t i = 0; i < f->n_px; ++i)   // (a depth is a positive distance or +inf: the minimum runs on the bits)
    if (!(host_depth[i] > 0.0f)) return set_error(RT_E_ARG, "rt_feat_add: a depth is not a positive distance or +inf");
  HIP_TRY(hipSetDevice(f->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  // one staging block: sums | hits | depth (freed when the call returns)
  const size_t sb = f->n_px * 6 * sizeof(uint64_t), wb = f->n_px * sizeof(uint32_t);
  DevBuf<char> stage;
  HIP_TRY(stage.alloc(sb + 2 * wb));
  hipError_t e = hipMemcpyAsync(stage.p, host_sums, sb, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(stage.p + sb, host_hits, wb, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(stage.p + sb + wb, host_depth, wb, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    const size_t blocks = std::max<size_t>(1, std::min<size_t>((f->n_px + 255) / 256, 4096));
    e = enqueue(feat_add_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, f->sums.p, f->hits.p,
                f->depth.p, reinterpret_cast<const unsigned long long*>(stage.p),
                reinterpret_cast<const unsigned*>(stage.p + sb), reinterpret_cast<const unsigned*>(stage.p + sb + wb),
                f->n_px);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e, "rt_feat_add");
  f->samples += samples;
  return RT_OK;
}

// The feature kernel a launch on ds would run under the current selector
// (diagnostic, tools/feat_time.py): out4 = {workgroups per CU, VGPRs per lane,
// LDS bytes per workgroup, the bodies' source: 0 tree in LDS, 1 tree in global
// memory, 2 linear scan}.
extern "C" int rt_feat_occupancy(const rt_dscene* ds, int* out4) {
  clear_error();
  if (!ds || !out4) return set_error(RT_E_ARG, "rt_feat_occupancy: NULL argument");
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::feat_source(si, selected_variant(), diag_build());
  if (const int rc = occupancy_report(feat_fn(src), kFeatThreads, policy::feat_lds(si, src), out4)) return rc;
  out4[3] = src;
  return RT_OK;
}

// ---- the body-id pass (rt.h, body_ids.h) --------------------------------------
static const void* ids_fn(int src) {
  return src == FEAT_LDS      ? reinterpret_cast<const void*>(&ids_kernel<FEAT_LDS>)
         : src == FEAT_GLOBAL ? reinterpret_cast<const void*>(&ids_kernel<FEAT_GLOBAL>)
                              : reinterpret_cast<const void*>(&ids_kernel<FEAT_SCAN>);
}

extern "C" int rt_launch_ids(const rt_dscene* ds, const rt_camera* c, int width, int rows, int row0, int32_t* d_ids,
                             void* hip_stream) {
  clear_error();
  const std::string me("rt_launch_ids");
  if (!ds || !c || !d_ids) return set_error(RT_E_ARG, me + ": NULL argument");
  if (const char* why = tp_shape_error(width, rows, row0)) return set_error(RT_E_ARG, me + ": " + why);
  // (the kernel's grid has a block row per kDnBy image rows)
  if ((rows + kDnBy - 1) / kDnBy > 65535) return set_error(RT_E_ARG, me + ": bad width/rows");
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device(me, stream, ds->device, "the scene")) return rc;
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::ids_source(si, selected_variant(), diag_build());
  const DTree& tr = ds->tree[1];
  IdsArgs a{};
  a.geo = ds->geo;
  a.blob = tr.blob;
  a.blob_f4 = tr.blob_f4;
  a.off_pairs = tr.off_pairs;
  a.off_pidx = tr.off_pidx;
  a.leaf_pairs = 2;
  a.big_pair0 = tr.big_pair0;
  a.n_big_leaves = tr.n_big_leaves;
  a.ref_mul = 1;   // (rt_scene_upload made the 4-body tree's inner refs byte offsets)
  for (int k = 0; k < 3; ++k) a.bvh_c[k] = tr.c[k];
  a.bvh_r = tr.r;
  a.bvh_c0 = tr.c0;
  ids_cam12(*c, a.cam);
  a.n = ds->n;
  a.width = width;
  a.rows = rows;
  a.row0 = row0;
  a.ids = d_ids;
  const dim3 grid(static_cast<unsigned>((width + kDnBx - 1) / kDnBx), static_cast<unsigned>((rows + kDnBy - 1) / kDnBy)),
      block(kDnBx, kDnBy);
  HIP_TRY(enqueue(ids_fn(src), grid, block, policy::feat_lds(si, src), stream, a));
  return RT_OK;
}

// The body-id kernel a launch on ds would run under the current selector
// (diagnostic, tools/motion_time.py): out4 as rt_feat_occupancy's.
extern "C" int rt_ids_occupancy(const rt_dscene* ds, int* out4) {
  clear_error();
  if (!ds || !out4) return set_error(RT_E_ARG, "rt_ids_occupancy: NULL argument");
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::ids_source(si, selected_variant(), diag_build());
  if (const int rc = occupancy_report(ids_fn(src), kFeatThreads, policy::feat_lds(si, src), out4)) return rc;
  out4[3] = src;
  return RT_OK;
}

// ---- ray queries (rt.h, ray_query.h) -------------------------------------------
static const void* rays_fn(int src, bool any) {
  if (any)
    return src == FEAT_LDS      ? reinterpret_cast<const void*>(&occluded_kernel<FEAT_LDS>)
           : src == FEAT_GLOBAL ? reinterpret_cast<const void*>(&occluded_kernel<FEAT_GLOBAL>)
                                : reinterpret_cast<const void*>(&occluded_kernel<FEAT_SCAN>);
  return src == FEAT_LDS      ? reinterpret_cast<const void*>(&rays_kernel<FEAT_LDS>)
         : src == FEAT_GLOBAL ? reinterpret_cast<const void*>(&rays_kernel<FEAT_GLOBAL>)
                              : reinterpret_cast<const void*>(&rays_kernel<FEAT_SCAN>);
}

// Both launches: the checks, then one kernel whose grid is the ray blocks, at
// most the workgroups the device holds at once (each stages the tree once and
// takes its blocks grid-stride).
static int launch_query(const char* who, bool any, const rt_dscene* ds, const rt_ray* d_rays, const int32_t* d_last,
                        size_t n, rt_ray_hit* d_hits, uint8_t* d_occ, void* hip_stream) {
  clear_error();
  const std::string me(who);
  if (!ds || (n > 0 && (!d_rays || (!d_hits && !d_occ)))) return set_error(RT_E_ARG, me + ": NULL argument");
  if ((reinterpret_cast<uintptr_t>(d_rays) | reinterpret_cast<uintptr_t>(d_hits)) & 15u)
    return set_error(RT_E_ARG, me + ": the rays and the hits must be 16-byte aligned");
  if (n > 0x7fffffffu) return set_error(RT_E_ARG, me + ": more than 2^31 - 1 rays");
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device(me, stream, ds->device, "the scene")) return rc;
  if (n == 0) return RT_OK;
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::ids_source(si, selected_variant(), diag_build());
  const size_t lds = policy::feat_lds(si, src);
  const void* fn = rays_fn(src, any);
  int per_cu = 0, cus = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kFeatThreads, lds));
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ds->device));
  const size_t resident = static_cast<size_t>(std::max(per_cu, 1)) * static_cast<size_t>(std::max(cus, 1));
  const size_t blocks = (n + kFeatThreads - 1) / kFeatThreads;
  const DTree& tr = ds->tree[1];
  RqArgs a{};
  a.geo = ds->geo;
  a.sph = ds->sph;
  a.blob = tr.blob;
  a.blob_f4 = tr.blob_f4;
  a.off_pairs = tr.off_pairs;
  a.off_pidx = tr.off_pidx;
  a.leaf_pairs = 2;
  a.big_pair0 = tr.big_pair0;
  a.n_big_leaves = tr.n_big_leaves;
  a.ref_mul = 1;   // (rt_scene_upload made the 4-body tree's inner refs byte offsets)
  for (int k = 0; k < 3; ++k) a.bvh_c[k] = tr.c[k];
  a.bvh_r = tr.r;
  a.bvh_c0 = tr.c0;
  a.n = ds->n;
  a.n_rays = static_cast<unsigned>(n);
  a.rays = reinterpret_cast<const float4*>(d_rays);
  a.last = d_last;
  a.hits = reinterpret_cast<float4*>(d_hits);
  a.occ = d_occ;
  HIP_TRY(enqueue(fn, dim3(static_cast<unsigned>(std::min(blocks, resident))), dim3(kFeatThreads), lds, stream, a));
  return RT_OK;
}

extern "C" int rt_launch_rays(const rt_dscene* ds, const rt_ray* d_rays, const int32_t* d_last, size_t n,
                              rt_ray_hit* d_hits, void* hip_stream) {
  return launch_query("rt_launch_rays", false, ds, d_rays, d_last, n, d_hits, nullptr, hip_stream);
}

extern "C" int rt_launch_occluded(const rt_dscene* ds, const rt_ray* d_rays, const int32_t* d_last, size_t n,
                                  uint8_t* d_occluded, void* hip_stream) {
  return launch_query("rt_launch_occluded", true, ds, d_rays, d_last, n, nullptr, d_occluded, hip_stream);
}

// The closest-hit kernel a launch on ds would run under the current selector
// (diagnostic, tools/rays_time.py): out4 as rt_feat_occupancy's.
extern "C" int rt_rays_occupancy(const rt_dscene* ds, int* out4) {
  clear_error();
  if (!ds || !out4) return set_error(RT_E_ARG, "rt_rays_occupancy: NULL argument");
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::ids_source(si, selected_variant(), diag_build());
  if (const int rc = occupancy_report(rays_fn(src, false), kFeatThreads, policy::feat_lds(si, src), out4)) return rc;
  out4[3] = src;
  return RT_OK;
}
