// dscene.h — the device scene (rt_dscene: the bodies, the three trees, the
// per-stream tile schedules, the refit state) and what the units bind to one:
// the policy's view of it, the trace unit's launch, selector and build kind,
// and the frame buffers that outlive the launches (FrameBuf: what rt_accum,
// rt_adapt, rt_budget and rt_feat share).  trace_kernel.h brings the standard
// headers the units use.
#pragma once
#include <mutex>
#include <vector>

#include "launch.h"
#include "trace_kernel.h"
#include "variant_policy.h"

namespace rtclj {

struct FillSet;   // trace.hip

// one BVH on the device: blob = nodes | pairs | pidx (the big bodies' leaves after the tree's)
struct DTree {
  float4* blob;
  int blob_f4, off_pairs, off_pidx, big_pair0, n_big_leaves, depth, n_nodes;
  float c[3], r;
  float c0;   // kPadRmax x the tree bodies' largest radius (bvh_pad.h)
};

// What rt_scene_update needs beyond the blobs (bvh_refit.h).  The host part is
// derived once at the upload; the device buffers and the staging are made by
// the first update, so a scene that is never updated pays for none of them.
constexpr int kRefitSlots = 4;
struct RefitState {
  std::vector<float> sph0;          // the upload's spheres: the preconditions' yardstick
  std::vector<int> bodies;          // the trees' bodies (one set for the three trees), ascending
  std::vector<int> order[3], lvl[3];   // tree_levels
  int empty = 0;                    // no body in the trees
  DevBuf<float4> src;               // the new spheres on the device
  DevBuf<int> d_order;              // order[0] | order[1] | order[2]
  // page-locked staging the caller's array is copied to, a ring: a slot is
  // reused once the copy out of it has run (its event)
  float* pin[kRefitSlots] = {};
  hipEvent_t ev[kRefitSlots] = {};
  int next = 0;
  bool ready = false;
  std::mutex mu;
  void release() {
    for (int i = 0; i < kRefitSlots; ++i) {
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      if (pin[i]) (void)hipHostFree(pin[i]);
      ev[i] = nullptr;
      pin[i] = nullptr;
    }
    src.reset();
    d_order.reset();
    ready = false;
  }
};

// Adaptive tile schedule (rt_launch): per stream, the per-tile durations of
// the stream's last launch and the longest-first order derived from them, for
// the launch shape `key` (frame rows, tiling, grid).  The order is a
// prediction: camera, spp, seed, flags and the kernel variant may change
// between launches of one shape (progressive passes, animation, A/B) and it
// stays a good one, and it never affects the result.  A launch of another
// shape re-keys the entry (and runs in dispatch order once).  Entries are per
// stream so that nothing a stream's kernels read is written from another
// stream; a dscene serves up to kSchedStreams streams this way, launches on
// further streams run unscheduled.
// The same per-stream entry holds the split tiles' partial sums (rt_launch).
// Its methods are rt_launch's stages (trace.hip, above launch_impl).
struct ScheduleKey {
  int width, rows, row_begin, row_tile, tile_first, tile_step, gx, gy;
};
struct Schedule {
  hipStream_t stream = nullptr;
  DevBuf<unsigned> cost;   // per tile
  DevBuf<int> order;       // per tile
  bool ready = false;      // order[] holds a permutation of key's tiles (stream-ordered)
  // The sort of the last launch's record (order_kernel, and plan_kernel for a
  // planned split) is enqueued at the start of the next launch of the shape
  // on the stream, not behind the trace kernel: a frame's launch ends with
  // its trace kernel (a one-frame process never pays the sort), and a frame
  // loop pays it once per frame as before.  sort_plan: the plan's unit count
  // (-1: no plan).
  bool sort_pending = false;
  int sort_plan = -1;
  ScheduleKey key{};
  DevBuf<unsigned long long> part;   // [rows][width][3] pixel sums of split tiles (zero between launches)
  // a split launch's trace kernel was enqueued but its finalize_kernel (which
  // re-zeroes the sums) was not: the next split launch zeroes them first
  bool part_dirty = false;
  // the stealing state (KArgs word, done, sum, owner, stealc)
  DevBuf<unsigned long long> word;     // per tile
  DevBuf<unsigned> done;               // per tile
  DevBuf<unsigned long long> sum;      // per tile x kPoolPx x 3, zero between uses
  DevBuf<int> owner;                   // KArgs n_owner entries
  DevBuf<unsigned long long> stealc;   // [helpers that got samples, their first samples] since rt_steal_stats
  unsigned epoch = 0;                  // launches with sharing on this stream (mod 2^16, 1 .. 65535)
  bool epoch_started = false;
  DevBuf<int2> units;                  // cost-balanced split plan (plan_kernel) of the next split launch
  int plan_units = -1;                 // the plan's unit count (-1: none)
  // path export (KArgs xq, xq_n): the records of a split launch's exported
  // paths (four uint4 each), and [written, the sweep's claims] (zeroed before each launch)
  DevBuf<uint4> xq;
  DevBuf<unsigned> xq_n;
  unsigned long long xq_launches = 0;   // export launches since rt_export_stats

  bool rekey(const ScheduleKey& k);
  int sort_record(int n_tiles, int spp);
  int bind_part(KArgs& a, size_t n_elems);
  int bind_order(KArgs& a, FillSet& fills, int n_tiles, int spp, int split_units, bool* first_order);
  int bind_sharing(KArgs& a, FillSet& fills, int n_tiles, int n_units, int slots, bool new_shape, bool first_order,
                   int64_t* grid);
  int bind_export(KArgs& a, FillSet& fills, size_t records);
  int record(int n_tiles, int spp, int plan_units_next);
};
constexpr int kSchedStreams = 16;
struct ScheduleSet {
  std::mutex mu;
  int used = 0;
  Schedule s[kSchedStreams];
  void release() {
    for (int k = 0; k < used; ++k) s[k] = Schedule{};
    used = 0;
  }
  // drop `stream`'s entry (its kernels have finished), keeping the others packed
  void release_stream(hipStream_t stream) {
    for (int k = 0; k < used; ++k)
      if (s[k].stream == stream) {
        if (k != used - 1) s[k] = std::move(s[used - 1]);
        s[used - 1] = Schedule{};
        --used;
        return;
      }
  }
  Schedule* find(hipStream_t stream) {
    for (int k = 0; k < used; ++k)
      if (s[k].stream == stream) return &s[k];
    return nullptr;
  }
  // `stream`'s entry, or a free one taken for it; NULL: every entry serves another stream
  Schedule* entry(hipStream_t stream) {
    Schedule* e = find(stream);
    if (e || used == kSchedStreams) return e;
    s[used].stream = stream;
    return &s[used++];
  }
};
}  // namespace rtclj

struct rt_dscene {
  int device;
  int n;
  int n_pad;
  float4* geo;
  float4* geo2;   // n_pad/2 Pairs (= n_pad float4)
  // BVHs (bvh.cpp): tree[0] 2-body leaves, tree[1] 4-body, tree[2] 8-body
  rtclj::DTree tree[3];
  float4* sph;
  float4* mat;
  int* kind;
  bool unit_albedo;            // every lambertian/metal albedo channel within [-1, 1] (compact_ok)
  uint64_t uid;                // upload id (scene_uid): contexts name scenes by it, not by address
  mutable rtclj::ScheduleSet sched;   // rt_launch's adaptive tile order
  rtclj::RefitState refit;            // rt_scene_update's
};

namespace rtclj {

// what the selection policy (variant_policy.h) reads of a scene, of a frame
inline policy::Scene scene_info(const rt_dscene& ds) {
  policy::Scene s{};
  for (int k = 0; k < 3; ++k) s.tree[k] = policy::Tree{ds.tree[k].n_nodes, ds.tree[k].depth, ds.tree[k].blob_f4};
  s.n_pad = ds.n_pad;
  s.unit_albedo = ds.unit_albedo;
  return s;
}
// The camera, sampler, seed key and row selection of a launch: the fields
// KArgs and FeatArgs share by name
template <class A>
void pack_frame(A& a, const rt_camera& c, const rt_params& p, int rows) {
  std::memcpy(a.cam + 0, c.center, 12);
  std::memcpy(a.cam + 3, c.p00, 12);
  std::memcpy(a.cam + 6, c.du, 12);
  std::memcpy(a.cam + 9, c.dv, 12);
  std::memcpy(a.cam + 12, c.disk_u, 12);
  std::memcpy(a.cam + 15, c.disk_v, 12);
  a.defocus = c.defocus ? 1 : 0;
  a.width = p.width;
  a.rows_out = rows;
  a.row_begin = p.row_begin;
  a.row_tile = p.row_tile > 0 ? p.row_tile : 8;
  a.tile_first = p.tile_first;
  a.tile_step = p.tile_step;
  a.spp = p.spp;
  a.sample_begin = p.sample_begin;
  // the loop-free samplers unless the caller asks for the reference's rejection loops
  a.sampler = (p.flags & RT_FLAG_REJECTION_SAMPLERS) ? 0 : (RT_SAMPLER_SPHERE | RT_SAMPLER_DISK);
  a.key = seed_key(p.seed);
}

// The trace unit's (trace.hip): the selector (rt_set_variant) and whether this
// is the diagnostic build, for the passes that follow the launch's choice; and
// rt_launch's body, which the accumulating passes share (acc_sums, active,
// units)
int selected_variant();
bool diag_build();
int launch_tile_rows(const rt_dscene& ds, const rt_params& p, int* vsel);
int launch_impl(const rt_dscene* ds, const rt_camera* c, const rt_params* p, float* d_out, uint64_t* d_counters,
                void* hip_stream, unsigned long long* acc_sums, const char* who = "rt_launch",
                const int* active = nullptr, int n_active = 0, const int2* units = nullptr, int n_units = 0);

// ---- frame buffers that outlive the launches (rt.h): what rt_accum, rt_adapt
// and rt_feat share.  Each is on its scene's device and holds a frame shape
// and the samples it has taken (host side; a pass counts when it is
// enqueued).  mu orders the count's updates and the entries' host state.
struct FrameBuf {
  int device = 0;
  rt_params shape{};   // width, height and the row selection (row_tile resolved)
  mutable std::mutex mu;
  int64_t samples = 0;
};
constexpr int64_t kAccumMaxSamples = 0xffffffffll;   // the sample index is a uint32

inline rt_params accum_shape(const rt_params& p) {
  rt_params s{};
  s.width = p.width;
  s.height = p.height;
  s.row_begin = p.row_begin;
  s.row_end = p.row_end;
  s.row_tile = p.row_tile > 0 ? p.row_tile : 8;
  s.tile_first = p.tile_first;
  s.tile_step = p.tile_step;
  return s;
}
inline bool same_shape(const rt_params& a, const rt_params& b) {
  return a.width == b.width && a.height == b.height && a.row_begin == b.row_begin && a.row_end == b.row_end &&
         a.row_tile == b.row_tile && a.tile_first == b.tile_first && a.tile_step == b.tile_step;
}
// a create's shape: *rows = its output rows (> 0)
inline int frame_rows(const char* who, const rt_params& shape, int* rows) {
  *rows = rows_out(shape);
  if (shape.width <= 0 || shape.height <= 0 || *rows <= 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad width/height/row selection");
  return RT_OK;
}
// a pass of p on ds into b (`noun`): the same device, the same shape
inline int check_match(const char* who, const char* noun, const FrameBuf& b, const rt_dscene& ds, const rt_params& p) {
  if (ds.device != b.device)
    return set_error(RT_E_ARG, std::string(who) + ": the scene is on device " + std::to_string(ds.device) + ", " + noun +
                                   " on device " + std::to_string(b.device));
  if (!same_shape(accum_shape(p), b.shape)) {
    const std::string n(noun);
    return set_error(RT_E_ARG, std::string(who) + ": width/height/row selection differ from " + n +
                                   (n.back() == 's' ? "'" : "'s"));
  }
  return RT_OK;
}
// ... and room for its samples (the caller holds b.mu)
inline int check_pass(const char* who, const char* noun, const FrameBuf& b, const rt_dscene& ds, const rt_params& p) {
  if (const int rc = check_match(who, noun, b, ds, p)) return rc;
  if (p.spp > 0 && b.samples + p.spp > kAccumMaxSamples)
    return set_error(RT_E_ARG, std::string(who) + ": more than 2^32 - 1 samples per pixel");
  return RT_OK;
}
// sums of `samples` samples per pixel added from the host (the caller holds b.mu)
inline int check_add(const char* who, const FrameBuf& b, int64_t samples) {
  if (samples < 0 || samples > kAccumMaxSamples || b.samples + samples > kAccumMaxSamples)
    return set_error(RT_E_ARG, std::string(who) + ": samples negative, or more than 2^32 - 1 per pixel in all");
  return RT_OK;
}
inline int64_t frame_samples(const FrameBuf* b) {
  if (!b) return 0;
  std::lock_guard<std::mutex> lk(b->mu);
  return b->samples;
}
// a create's new buffer object for `shape` on ds's device, which is made current
template <class B>
inline int frame_new(const rt_dscene& ds, const rt_params& shape, B** b) {
  HIP_TRY(hipSetDevice(ds.device));
  *b = new B;
  (*b)->device = ds.device;
  (*b)->shape = accum_shape(shape);
  return RT_OK;
}
// ... handed out once its allocations and first fills (e) are done: the first
// pass may come on any stream
template <class B>
inline int frame_created(const char* who, B* b, hipError_t e, B** out) {
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    delete b;
    return hip_fail(e, who);
  }
  *out = b;
  return RT_OK;
}
template <class B>
inline int frame_free(B* b) {
  if (!b) return RT_OK;
  (void)hipSetDevice(b->device);
  delete b;
  return RT_OK;
}
inline int check_resolve_flags(const char* who, int flags) {
  if ((flags & ~(RT_FLAG_REALM | RT_FLAG_STREAMED | RT_FLAG_REJECTION_SAMPLERS)) != 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad flags");
  return RT_OK;
}
}  // namespace rtclj
