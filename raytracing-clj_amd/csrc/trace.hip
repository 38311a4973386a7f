// trace.hip — the trace unit: what a plain frame launches.  The shipped
// kernel's instantiations (trace_kernel.h: the default BVH walk in its two LDS
// images and its fallbacks), the schedule / split / fill / quantise kernels,
// and rt_scene_upload / rt_launch / rt_prepare with the variant selection
// (variant_policy.h's pure functions), the per-stream tile schedule and the
// stats, steal, export, schedule and debug entries.  Built twice: with
// -DRTCLJ_DIAG it looks up the A/B scans, the direction-coherent waves and the
// statistics builds of trace_diag.hip (librtclj_diag.so only).  DESIGN.md §3.
// The other units (frames.hip, first_hit.hip, image.hip, refit.hip) reach it
// through launch.h and dscene.h.
#include "trace_kernel.h"
#include "first_hit.h"
#include "bvh_refit.h"
#include "dscene.h"

namespace rtclj {

// The adaptive schedule's sort: tile indices by descending cost (a counting
// sort over 256 log-scale buckets: the top 5 bits are the cost's bit length,
// the low 3 the bits below its leading one).  One block; the order within a
// bucket is arbitrary (any order renders the same bits).  Each cost is then
// halved, so the next launch sorts by its own durations plus half of this
// history (a decayed mean: a tile's cost depends on what shared its CU;
// profiles/r02/shard_cost_decay.txt).
__device__ __forceinline__ int cost_bucket(unsigned c) {
  if (c < 8) return static_cast<int>(c);
  const int e = 31 - __clz(c);                                  // 3..31
  return ((e - 2) << 3) | static_cast<int>((c >> (e - 3)) & 7u); // monotone, < 256
}
__global__ __launch_bounds__(1024) void order_kernel(unsigned* __restrict__ cost, int* __restrict__ order,
                                                     int n) {
  __shared__ int hist[256];
  __shared__ int cursor[256];
  __shared__ int scan[256];
  const int t = static_cast<int>(threadIdx.x);
  if (t < 256) hist[t] = 0;
  __syncthreads();
  for (int i = t; i < n; i += 1024) atomicAdd(&hist[cost_bucket(cost[i])], 1);
  __syncthreads();
  // descending cost first: bucket b's first slot is the count of the buckets
  // above it (a parallel scan over the reversed histogram, 8 steps)
  if (t < 256) scan[t] = hist[255 - t];
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = (t < 256 && t >= off) ? scan[t - off] : 0;
    __syncthreads();
    if (t < 256) scan[t] += v;
    __syncthreads();
  }
  if (t < 256) cursor[255 - t] = scan[t] - hist[255 - t];
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 1024) {
    const unsigned c = cost[i];
    order[atomicAdd(&cursor[cost_bucket(c)], 1)] = i;
    cost[i] = c >> 1;   // the next launch adds its durations to half of these
  }
}

// The split tiles' pixels (order positions [n_whole, n_tiles)): the sum of
// their splits' integer sums (added by the splits' atomics: exact, any
// order), then the unsplit epilogue's conversion: RN(float(sum)) * 2^-24,
// / spp (realm: * (1/spp)); the sums are zeroed for the next launch.  One
// block per split tile, thread t = tile row * 24 + x * 3 + channel.
__global__ __launch_bounds__(384) void finalize_kernel(unsigned long long* __restrict__ part,
                                                        const int* __restrict__ order, int n_whole,
                                                        int tiles_x, int tile_h, int width, int rows,
                                                        float* __restrict__ out, int spp, int realm) {
  const int pos = n_whole + static_cast<int>(blockIdx.x);
  const int tile = order ? order[pos] : pos;
  const int tby = tile / tiles_x, tbx = tile - tby * tiles_x;
  const int t = static_cast<int>(threadIdx.x);
  const int row = t / (kTile * 3), col = t - row * (kTile * 3);
  const int y = tby * tile_h + row, x3 = tbx * kTile * 3 + col;
  if (row >= tile_h || y >= rows || x3 >= width * 3) return;
  const size_t e = static_cast<size_t>(y) * width * 3 + x3;
  const unsigned long long sum = part[e];
  part[e] = 0ull;
  const float tot = static_cast<float>(sum) * 0x1p-24f;
  const float inv = static_cast<float>(spp > 0 ? spp : 1);
  out[e] = realm ? tot * (1.0f / inv) : tot / inv;
}

// The library's own buffer fill (zeroing the per-stream records, the split
// sums, the counters): every memset of the product path runs this kernel, in
// the library's code object, instead of the HIP runtime's blit kernel, whose
// code object a fresh process would otherwise load on its first frame.
__global__ __launch_bounds__(256) void fill_kernel(uint32_t* __restrict__ p, uint32_t v, size_t n) {
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) p[i] = v;
}

// Several fills in one launch: the zeroings a launch of a new shape needs
// (its tile-cost record, the sharing words and owner table) as one kernel in
// front of the trace kernel instead of one small launch each.
struct FillSet {
  static constexpr int kMax = 6;
  uint32_t* p[kMax];
  uint32_t v[kMax];
  size_t n[kMax];
  int count = 0;
  void add(void* ptr, int byte_value, size_t bytes) {
    p[count] = static_cast<uint32_t*>(ptr);
    v[count] = static_cast<uint32_t>(byte_value & 0xff) * 0x01010101u;
    n[count] = bytes / 4;
    ++count;
  }
};
// A shape's first order, before any record: the tiles bottom-up
// (order[i] = n - 1 - i)
__global__ __launch_bounds__(256) void iota_rev_kernel(int* __restrict__ order, int n) {
  const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (i < n) order[i] = n - 1 - i;
}

__global__ __launch_bounds__(256) void fill_set_kernel(const FillSet f) {
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (int k = 0; k < f.count; ++k)
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < f.n[k]; i += stride) f.p[k][i] = f.v[k];
}

// rt_quantize on the device (rt_render_u8, rt_quantize_device): a channel's
// byte is the number of thresholds t[1..255] <= it (rt_internal.h), found by
// an 8-step binary search in LDS -- NaN fails every compare and gets 0, as
// rt_quantize's isnan does.  Streaming: 4 bytes read, 1 written per channel.
__global__ __launch_bounds__(256) void quantize_kernel(const float* __restrict__ lin, uint8_t* __restrict__ out,
                                                        size_t n, const QThr q) {
  __shared__ float s_t[256];
  s_t[threadIdx.x] = q.t[threadIdx.x];
  __syncthreads();
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
    const float c = lin[i];
    int b = 0;
#pragma unroll
    for (int step = 128; step > 0; step >>= 1)
      if (s_t[b + step] <= c) b += step;   // b + step <= 255
    out[i] = static_cast<uint8_t>(b);
  }
}

// Cost-balanced splits: the next split launch of the shape deals its U units
// to the tiles in proportion to their recorded cost (the decayed record
// order_kernel has just sorted and halved), so that units cost about the
// same and the launch does not end on a few long ones (a uniform split of
// C1's 8-GPU shard left units of 330-360 us against a 259 us mean in the
// launch's tail: DESIGN.md §6).  Tile at order position p gets
// s_p = min(smax, 1 + floor(cost_p (U - n) / C)) units, the U - sum s units
// left go one each to the first positions, and unit u of the plan is
// {tile, k | s << 8}: samples [k spp / s, (k + 1) spp / s).  Units the clamps
// leave over are {-1, 0}.  One block.
__global__ __launch_bounds__(1024) void plan_kernel(const unsigned* __restrict__ cost, const int* __restrict__ order,
                                                     int n, int U, int smax, int2* __restrict__ units) {
  __shared__ unsigned long long s_tot;
  __shared__ int s_part[1024];
  __shared__ int s_left;
  const int tid = static_cast<int>(threadIdx.x);
  const int per = (n + 1023) / 1024;
  const int p0 = min(n, tid * per), p1 = min(n, p0 + per);
  if (tid == 0) s_tot = 0ull;
  __syncthreads();
  unsigned long long my = 0;
  for (int p = p0; p < p1; ++p) my += cost[order[p]];
  if (my) atomicAdd(&s_tot, my);
  __syncthreads();
  const unsigned long long tot = s_tot;
  const int spare = max(0, U - n);
  auto raw = [&](int p) {
    const long long c = static_cast<long long>(cost[order[p]]);
    const long long extra = tot ? (c * spare) / static_cast<long long>(tot) : spare / max(n, 1);
    return static_cast<int>(min<long long>(smax, 1 + extra));
  };
  int sum = 0;
  for (int p = p0; p < p1; ++p) sum += raw(p);
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int i = 0; i < 1024; ++i) t += s_part[i];
    s_left = max(0, U - t);
  }
  __syncthreads();
  const int left = s_left;
  auto fin = [&](int p) {
    const int r = raw(p);
    return r + ((p < left && r < smax) ? 1 : 0);
  };
  sum = 0;
  for (int p = p0; p < p1; ++p) sum += fin(p);
  __syncthreads();
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {   // exclusive prefix of the threads' unit counts (1024 adds)
    int run = 0;
    for (int i = 0; i < 1024; ++i) {
      const int v = s_part[i];
      s_part[i] = run;
      run += v;
    }
    s_left = run;   // units used
  }
  __syncthreads();
  int base = s_part[tid];
  for (int p = p0; p < p1; ++p) {
    const int sp = fin(p);
    const int tile = order[p];
    for (int k = 0; k < sp; ++k) units[base + k] = make_int2(tile, k | (sp << 8));
    base += sp;
  }
  for (int u = s_left + tid; u < U; u += 1024) units[u] = make_int2(-1, 0);
}

// ------------------------------------------------------------- host ------
// Kernel variants (rt_set_variant): variant_policy.h lists them and holds each
// one's traits; its kernel is looked up here, and in trace_diag.hip for what
// only the diagnostic library (lib/librtclj_diag.so) carries.
#ifdef RTCLJ_DIAG
constexpr bool kDiag = true;
#else
constexpr bool kDiag = false;
#endif
// the policy's copies of the kernels' shapes, and its table's columns against
// trace_kernel.h's traits of each row's scan
static_assert(policy::kTile == kTile && policy::kPoolPx == kPoolPx && policy::kXBytes == kXBytes,
              "variant_policy.h: the kernels' shapes");
constexpr bool traits_agree() {
  for (const policy::Traits& t : policy::kTraits) {
    if (t.build == policy::BUILD_NONE) continue;
    const int walk = t.scan == SCAN_BVHS ? policy::WALK_SORTED : is_bvh_scan(t.scan) ? policy::WALK_BVH : policy::WALK_NONE;
    if (t.walk != walk || t.tree != scan_tree(t.scan) || t.compact != is_compact_scan(t.scan) ||
        t.entry_bytes != stack_entry_bytes(t.scan) || policy::variant_rows(t) != (t.th ? t.th : tile_rows(t.scan)) ||
        (walk == policy::WALK_SORTED && t.threads != kSortThreads))
      return false;
  }
  return true;
}
static_assert(traits_agree(), "variant_policy.h: a row's columns against its scan's traits");

const void* trace_kernel_w16();   // trace_w16.hip
static const policy::Traits& variant_traits(int v) { return policy::traits(v, kDiag); }
static const void* variant_fn(int v) {
  switch (v) {
    case policy::kDefault: return RT_K(SRC_LDS, SCAN_BVHQ, false);   // (resolved per scene)
    case policy::kScan: return RT_K(SRC_SCALAR, SCAN_GROUP4, false);
    case policy::kGlobal: return RT_K(SRC_SCALAR, SCAN_BVH, false);
    case policy::kFull4: return RT_K(SRC_LDS, SCAN_BVHQ, false);
    case policy::kLeaf8: return RT_KW(SRC_LDS, SCAN_BVHO, false, 8);
    case policy::kCompact: return reinterpret_cast<const void*>(&trace_kernel<SRC_LDS, SCAN_BVHQ7, false, 4, 0, false, true>);
    case policy::kCompactW8: return RT_KW(SRC_LDS, SCAN_BVHQ7, false, 8);
    case policy::kCompactW16: return trace_kernel_w16();   // (trace_w16.hip, compiled with its own scheduler flag)
    case policy::kCompactTh4: return RT_KWT(SRC_LDS, SCAN_BVHQ7, false, 4, 4);
    case policy::kCompactWalk: return RT_K(SRC_LDS, SCAN_BVHQ7, false);
  }
#ifdef RTCLJ_DIAG
  return diag_kernel(v);
#else
  return nullptr;
#endif
}
// the variant's sweep kernel (path export, KArgs::xq), or NULL
static const void* variant_sweep(int v) { return v == policy::kCompact ? RT_KSW(SRC_LDS, SCAN_BVHQ7, 4, 0) : nullptr; }

// selectors (rt_set_variant / rt_set_schedule): atomics, read once per launch
static std::atomic<int> g_variant{0};
// tile schedule: 0 = adaptive longest-first, 1 = dispatch order
static std::atomic<int> g_schedule{0};
// BVH build: surface-area splits (default) or median splits (RTCLJ_BVH=median,
// for A/B): tree_blob.cpp's bvh_sah_default
static const bool g_bvh_sah = bvh_sah_default();
#ifdef RTCLJ_DIAG
// diagnostic build: RTCLJ_TIMELINE=1 records every launch's wave timeline
static const bool g_timeline = [] {
  const char* e = std::getenv("RTCLJ_TIMELINE");
  return e && std::atoi(e) != 0;
}();
#endif
// stats builds: per device, u64[kDbg] event counters and the u64[4 * kDbgWaves]
// wave timeline, allocated on that device at its first stats launch
constexpr int kDbg = 40;   // (rt_debug_stats reads the first 32, rt_debug_stats_ext all)
constexpr int kDbgDevices = 64;
static std::mutex g_dbg_mu;
static unsigned long long* g_dbg[kDbgDevices] = {};
static unsigned long long* g_dbgw[kDbgDevices] = {};

// what the other units' passes read of the two (dscene.h)
int selected_variant() { return g_variant.load(); }
bool diag_build() { return kDiag; }

}  // namespace rtclj

using namespace rtclj;

hipError_t rtclj::fill_words(void* p, uint32_t word, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const size_t blocks = std::min<size_t>((n + 255) / 256, 2048);
  return enqueue(fill_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, static_cast<uint32_t*>(p), word, n);
}

namespace rtclj {
int fill_async(void* p, int byte_value, size_t bytes, void* stream) {
  if (bytes % 4 != 0) return hipErrorInvalidValue;   // (every buffer the product fills is whole words)
  return fill_words(p, static_cast<uint32_t>(byte_value & 0xff) * 0x01010101u, bytes / 4, static_cast<hipStream_t>(stream));
}

int quantize_launch(const float* d_lin, uint8_t* d_out, size_t n, void* stream) {
  if (n == 0) return hipSuccess;
  const size_t blocks = std::min<size_t>((n + 255) / 256, 4096);
  return enqueue(quantize_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), d_lin,
                 d_out, n, quantize_table());
}
}  // namespace rtclj

static std::atomic<uint64_t> g_scene_uid{0};
uint64_t rtclj::scene_uid(const rt_dscene* ds) { return ds ? ds->uid : 0; }

// live device scenes, for release_stream_schedules (rt_host.cpp's contexts)
static std::mutex g_scenes_mu;
static std::vector<rt_dscene*> g_scenes;

// the live scenes among `uids` (a context's list may name freed ones; a
// new scene at a freed one's address has another id)
template <class F>
static void for_live_scenes(const uint64_t* uids, int n, F f) {
  std::lock_guard<std::mutex> lk(g_scenes_mu);
  for (rt_dscene* d : g_scenes)
    if (std::find(uids, uids + n, d->uid) != uids + n) {
      std::lock_guard<std::mutex> l2(d->sched.mu);
      f(d->sched);
    }
}

void rtclj::release_stream_schedules(void* stream, const uint64_t* uids, int n) {
  for_live_scenes(uids, n, [&](ScheduleSet& set) { set.release_stream(static_cast<hipStream_t>(stream)); });
}

void rtclj::rebind_stream_schedules(void* from, void* to, const uint64_t* uids, int n) {
  for_live_scenes(uids, n, [&](ScheduleSet& set) {
    Schedule* src = nullptr;
    for (int k = 0; k < set.used; ++k) {
      if (set.s[k].stream == static_cast<hipStream_t>(to)) return;
      if (set.s[k].stream == static_cast<hipStream_t>(from)) src = &set.s[k];
    }
    if (src) src->stream = static_cast<hipStream_t>(to);
  });
}

extern "C" int rt_set_variant(int v) {
  clear_error();
  if (!policy::has_variant(v, kDiag))
    return set_error(RT_E_ARG, "rt_set_variant: variant " + std::to_string(v) +
                                   " is not in this build (diagnostic variants: lib/librtclj_diag.so)");
  return g_variant.exchange(v);
}

extern "C" int rt_set_schedule(int mode) {
  clear_error();
  if (mode != 0 && mode != 1) return set_error(RT_E_ARG, "rt_set_schedule: mode must be 0 or 1");
  return g_schedule.exchange(mode);
}

extern "C" int rt_scene_upload(int device, const rt_scene* s, rt_dscene** out) {
  clear_error();
  if (!s || !out) return set_error(RT_E_ARG, "rt_scene_upload: NULL argument");
  *out = nullptr;
  if (s->n < 0 || (s->n > 0 && (!s->sphere || !s->mat_kind || !s->mat)))
    return set_error(RT_E_ARG, "rt_scene_upload: bad scene arrays");
  if (s->n > RT_MAX_SPHERES)
    return set_error(RT_E_TOO_MANY, "rt_scene_upload: " + std::to_string(s->n) +
                                        " spheres > RT_MAX_SPHERES (" +
                                        std::to_string(RT_MAX_SPHERES) + ")");
  for (int i = 0; i < s->n; ++i) {
    const int k = s->mat_kind[i];
    if (k != RT_LAMBERTIAN && k != RT_METAL && k != RT_DIELECTRIC && k != RT_NONE)
      return set_error(RT_E_MATERIAL, "rt_scene_upload: body " + std::to_string(i) +
                                          " has unsupported material kind " + std::to_string(k));
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return set_error(RT_E_NODEV, "rt_scene_upload: device " + std::to_string(device) +
                                     " not available (" + std::to_string(ndev) + " visible)");
  HIP_TRY(hipSetDevice(device));
  const int n = s->n;
  const int n_pad = ((n + 3) / 4) * 4 + 4;   // grouped scan reads up to 4 past the last group
  const size_t cnt = n > 0 ? n : 1;
  // pads: -r^2 = +inf -> c = +inf, disc = -inf: never a candidate
  std::vector<float4> geo(n_pad, make_float4(0.0f, 0.0f, 0.0f, INFINITY)), sph(cnt), mat(cnt);
  std::vector<int> kind(cnt, 0);
  for (int i = 0; i < n; ++i) {
    const float* q = s->sphere + 4 * i;
    const float r = q[3];
    float g[4];
    fh_geo(q, g);   // (centre, -r^2): first_hit.h's, which rt_ids_host builds too
    geo[i] = make_float4(g[0], g[1], g[2], g[3]);
    sph[i] = make_float4(q[0], q[1], q[2], 1.0f / r);                   // 1/r for the normal
    const float* m = s->mat + 4 * i;
    mat[i] = make_float4(m[0], m[1], m[2], m[3]);
    if (s->mat_kind[i] == RT_DIELECTRIC) {   // (albedo unused)
      mat[i].x = 1.0f / m[3];                // ri of a front face: 1/eta
      // Schlick's r0 = ((1 - ri) / (1 + ri))^2 for ri = 1/eta (front face) and
      // eta (back face): the kernel's fp32 ops, done once here (IEEE division,
      // no contraction: the same bits)
      for (int f = 0; f < 2; ++f) {
        const float ri = f == 0 ? mat[i].x : m[3];
        float r0 = (1.0f - ri) / (1.0f + ri);
        r0 = r0 * r0;
        (f == 0 ? mat[i].y : mat[i].z) = r0;
      }
    }
    kind[i] = s->mat_kind[i];
  }
  // pair-interleaved copy for the packed scan: (x0 x1 y0 y1 z0 z1 w0 w1) per pair
  std::vector<float> geo2(4 * static_cast<size_t>(n_pad));
  for (int q = 0; q < n_pad / 2; ++q) {
    const float4 b0 = geo[2 * q], b1 = geo[2 * q + 1];
    float* o = &geo2[8 * static_cast<size_t>(q)];
    o[0] = b0.x; o[1] = b1.x; o[2] = b0.y; o[3] = b1.y;
    o[4] = b0.z; o[5] = b1.z; o[6] = b0.w; o[7] = b1.w;
  }
  rt_dscene* d = new rt_dscene{};
  d->uid = ++g_scene_uid;
  d->device = device;
  d->n = n;
  d->n_pad = n_pad;
  d->unit_albedo = true;
  for (int i = 0; i < n; ++i)
    if (s->mat_kind[i] == RT_LAMBERTIAN || s->mat_kind[i] == RT_METAL)
      for (int c = 0; c < 3; ++c)
        if (!(std::fabs(s->mat[4 * i + c]) <= 1.0f)) d->unit_albedo = false;
  // BVHs over the bodies (the traversal variants), the three trees built
  // concurrently on host threads (C1: 2.4 -> ~1 ms of a first rt_render)
  BvhHost bvhs[3];
  {
    std::thread th[2];
    for (int k = 1; k < 3; ++k) th[k - 1] = std::thread([&, k] { bvh_build(s->sphere, n, &bvhs[k], 2 << k, g_bvh_sah); });
    bvh_build(s->sphere, n, &bvhs[0], 2, g_bvh_sah);
    for (std::thread& t : th) t.join();
  }
  hipError_t e = hipMalloc(&d->geo, n_pad * sizeof(float4));
  // blob = nodes | pairs | pidx (tree_blob.cpp's tree_pack: rt_tree_build_host's bytes)
  for (int k = 0; k < 3 && e == hipSuccess; ++k) {
    std::vector<char> blob;
    rt_tree_info ti;
    tree_pack(bvhs[k], k, &blob, &ti);
    DTree& t = d->tree[k];
    t.blob_f4 = static_cast<int>(blob.size() / 16);
    t.off_pairs = ti.off_pairs;
    t.off_pidx = ti.off_pidx;
    t.big_pair0 = ti.big_pair0;
    t.n_big_leaves = ti.n_big_leaves;
    t.depth = ti.depth;
    t.n_nodes = ti.n_nodes;
    for (int j = 0; j < 3; ++j) t.c[j] = ti.center[j];
    t.r = ti.radius;
    t.c0 = ti.c0;
    // what a refit walks (rt_scene_update), from the bytes the device gets
    tree_levels(blob.data(), ti, &d->refit.order[k], &d->refit.lvl[k]);
    if (k == 0) {
      d->refit.bodies = tree_bodies(blob.data(), ti);
      d->refit.empty = d->refit.bodies.empty();
    }
    e = hipMalloc(&t.blob, blob.size());
    if (e == hipSuccess) e = hipMemcpy(t.blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
  }
  if (n > 0) d->refit.sph0.assign(s->sphere, s->sphere + 4 * static_cast<size_t>(n));
  if (e == hipSuccess) e = hipMalloc(&d->geo2, n_pad * sizeof(float4));
  if (e == hipSuccess) e = hipMemcpy(d->geo2, geo2.data(), n_pad * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&d->sph, cnt * sizeof(float4));
  if (e == hipSuccess) e = hipMalloc(&d->mat, cnt * sizeof(float4));
  if (e == hipSuccess) e = hipMalloc(&d->kind, cnt * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(d->geo, geo.data(), n_pad * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d->sph, sph.data(), cnt * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d->mat, mat.data(), cnt * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d->kind, kind.data(), cnt * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    rt_scene_free(d);
    return hip_fail(e, "rt_scene_upload");
  }
  {
    std::lock_guard<std::mutex> lk(g_scenes_mu);
    g_scenes.push_back(d);
  }
  *out = d;
  return RT_OK;
}

extern "C" int rt_scene_free(rt_dscene* d) {
  if (!d) return RT_OK;
  {
    std::lock_guard<std::mutex> lk(g_scenes_mu);
    g_scenes.erase(std::remove(g_scenes.begin(), g_scenes.end(), d), g_scenes.end());
  }
  (void)hipSetDevice(d->device);
  if (d->geo) (void)hipFree(d->geo);
  if (d->geo2) (void)hipFree(d->geo2);
  for (const DTree& t : d->tree) {
    if (t.blob) (void)hipFree(t.blob);
  }
  d->sched.release();
  d->refit.release();
  if (d->sph) (void)hipFree(d->sph);
  if (d->mat) (void)hipFree(d->mat);
  if (d->kind) (void)hipFree(d->kind);
  delete d;
  return RT_OK;
}

// workgroups device `device` holds at once for kernel fn with `lds` bytes of
// dynamic LDS (CUs x the occupancy query), cached per (device, fn, lds)
static int launch_slots(int device, const void* fn, size_t lds, int threads = 256) {
  struct Entry { int device; const void* fn; size_t lds; int slots; };
  static std::mutex mu;
  static std::vector<Entry> cache;
  std::lock_guard<std::mutex> lk(mu);
  for (const Entry& e : cache)
    if (e.device == device && e.fn == fn && e.lds == lds) return e.slots;
  int cus = 0, per = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, threads, lds) != hipSuccess)
    return 0;
  cache.push_back({device, fn, lds, cus * per});
  return cus * per;
}

// the variant a launch of p on ds runs under the current selector
static int launch_variant(const rt_dscene& ds, const rt_params& p) {
  const int sel = g_variant.load();
  const policy::Scene s = scene_info(ds);
  const policy::Frame f{p.width, p.height, rows_out(p), p.spp};
  int vsel = policy::launch_variant(s, f, sel, kDiag, 0, 0);
  // RTCLJ_TH4 (policy::launch_variant): read, and the device asked for 22's
  // resident workgroups, only where the default runs 22
  if (sel == policy::kDefault && vsel == policy::kCompact) {
    const int ratio = env_int("RTCLJ_TH4", 0, 0);
    if (ratio > 0) {
      const int threads = variant_traits(vsel).threads;
      const int slots = launch_slots(ds.device, variant_fn(vsel), policy::lds_of_compact(s.tree[1], threads), threads);
      vsel = policy::launch_variant(s, f, sel, kDiag, ratio, slots);
    }
  }
  return vsel;
}

extern "C" int rt_resolve_variant(const rt_dscene* ds) {
  return ds ? policy::resolve_variant(scene_info(*ds), g_variant.load(), kDiag) : -1;
}

// Occupancy of the launch rt_launch would make for (ds, p): the HIP occupancy
// query on the kernel and dynamic LDS it would use (diagnostic, bench.py).
extern "C" int rt_launch_occupancy(const rt_dscene* ds, const rt_params* p, int* out4) {
  clear_error();
  if (!ds || !p || !out4) return set_error(RT_E_ARG, "rt_launch_occupancy: NULL argument");
  const int rows = rows_out(*p);
  if (rows <= 0 || p->width <= 0) return set_error(RT_E_ARG, "rt_launch_occupancy: empty frame");
  HIP_TRY(hipSetDevice(ds->device));
  const int vsel = launch_variant(*ds, *p);
  const void* fn = variant_fn(vsel);
  if (!fn) return set_error(RT_E_ARG, "rt_launch_occupancy: no kernel for variant " + std::to_string(vsel));
  const size_t lds = policy::launch_lds(scene_info(*ds), vsel, kDiag);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  const int threads = variant_traits(vsel).threads;
  if (const int rc = occupancy_report(fn, threads, lds, out4)) return rc;
  out4[0] = out4[0] * threads / 256;   // (in 256-thread workgroups) per CU
  out4[3] = vsel;
  return RT_OK;
}

static int dbg_buffers(int device, unsigned long long** dbg, unsigned long long** dbgw) {
  if (device < 0 || device >= kDbgDevices) return set_error(RT_E_ARG, "stats launch: device index too large");
  std::lock_guard<std::mutex> lk(g_dbg_mu);
  if (!g_dbg[device]) {
    HIP_TRY(hipMalloc(&g_dbg[device], kDbg * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(g_dbg[device], 0, kDbg * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(&g_dbgw[device], 4 * kDbgWaves * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(g_dbgw[device], 0, 4 * kDbgWaves * sizeof(unsigned long long)));
  }
  *dbg = g_dbg[device];
  *dbgw = g_dbgw[device];
  return RT_OK;
}

// ceil(2^64 / d), 0 for d <= 1: n / d = the high half of n * m for every
// 32-bit n (m * d = 2^64 + e with e < d, so n * e < 2^64 never reaches the
// quotient)
static uint64_t magic64(int d) { return d <= 1 ? 0 : ~0ull / static_cast<uint64_t>(d) + 1ull; }

// ---- rt_launch's stages ----------------------------------------------------
// The variant a launch runs: its number, traits and kernels
struct Kernel {
  int vsel;
  policy::Traits t;
  const void* fn;
  const void* sweep;
};
// ... chosen for a launch of p on ds
static int bound_variant(const rt_dscene& ds, const rt_params& p) {
  const int vsel = launch_variant(ds, p);
  if (variant_traits(vsel).walk == policy::WALK_SORTED && p.max_depth > 1023)
    return policy::kFull4;   // (a path's depth left: 10 bits in the exchange)
  return vsel;
}

// ... and its tile rows: what a caller that enqueues work of its own ahead of a
// list or unit-table pass asks first, so that the pass's refusal finds nothing
// enqueued
int rtclj::launch_tile_rows(const rt_dscene& ds, const rt_params& p, int* vsel) {
  *vsel = bound_variant(ds, p);
  return policy::variant_rows(variant_traits(*vsel));
}

// ... and its tree and stack bound to the arguments
static int bind_variant(const char* who, const rt_dscene& ds, const rt_params& p, KArgs& a, Kernel* out) {
  const int vsel = bound_variant(ds, p);
  const Kernel v{vsel, variant_traits(vsel), variant_fn(vsel), variant_sweep(vsel)};
  if (!v.fn) return set_error(RT_E_ARG, std::string(who) + ": no kernel for variant " + std::to_string(vsel));
  const DTree& tr = ds.tree[v.t.tree];
  a.bvh_blob = tr.blob;
  a.bvh_blob_f4 = tr.blob_f4;
  a.bvh_off_pairs = tr.off_pairs;
  a.bvh_off_pidx = tr.off_pidx;
  a.big_pair0 = tr.big_pair0;
  a.n_big_leaves = tr.n_big_leaves;
  a.bvh_stack = policy::launch_stack(scene_info(ds), v.t);
  for (int k = 0; k < 3; ++k) a.bvh_c[k] = tr.c[k];
  a.bvh_r = tr.r;
  a.bvh_c0 = tr.c0;
  // drain compaction: a post holds as many paths as a wave's stack slice has
  // room for (RTCLJ_COMPACT: post at or below that many paths; 0 off)
  const int words = a.bvh_stack * 16 * v.t.entry_bytes;   // a wave's stack slice
  a.mb_paths = std::min(32, words / kMbFields);
  a.compact = is_bvh_scan(v.t.scan) ? std::min(a.mb_paths, env_int("RTCLJ_COMPACT", a.mb_paths, 0)) : 0;
  *out = v;
  return RT_OK;
}

// the statistics builds' counters and the wave timeline
static int bind_debug(int device, const Kernel& v, KArgs& a) {
  if (v.t.stats) return dbg_buffers(device, &a.dbg, &a.dbgw);
#ifdef RTCLJ_DIAG
  if (g_timeline) {   // wave timeline only (rt_debug_waves), no counters
    unsigned long long* unused = nullptr;
    return dbg_buffers(device, &unused, &a.dbgw);
  }
#endif
  return RT_OK;
}

// the launch's dynamic LDS, allowed for on the variant's kernels
static int bind_lds(const rt_dscene& ds, const Kernel& v, size_t* out) {
  size_t lds = policy::launch_lds(scene_info(ds), v.vsel, kDiag);
#ifdef RTCLJ_DIAG
  // (diagnostic: RTCLJ_LDS_PAD bytes of dynamic LDS added to the launch, to
  // measure the kernel at fewer workgroups per CU)
  lds += static_cast<size_t>(env_int("RTCLJ_LDS_PAD", 0, 0));
#endif
  if (lds > 64 * 1024) {
    HIP_TRY(hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    if (v.sweep) HIP_TRY(hipFuncSetAttribute(v.sweep, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  }
  *out = lds;
  return RT_OK;
}

// Sample split: a frame of fewer tiles than
// kSplitRounds x the workgroups the GPU holds at once (a shard of a
// multi-GPU frame, a small image) runs every tile as `split` workgroups,
// one contiguous sample range each, so that the launch does not end on a
// few whole tiles running alone (its length would be the longest tile's).
// The integer pixel sums add up to the same bits in any grouping.
// (The kernel also takes a whole-tile prefix of the order, n_whole; the
// split tiles' partial sums go through finalize_kernel.)
// (Tile sharing, below, takes the launches that are not split: a split
// launch has about one unit per workgroup slot, all of which end together,
// and on C1's 8-GPU shard the split is faster -- 1.05 vs 1.09-1.18 ms --
// while sharing balances the tail of a long launch in plain order, C1
// 6.78 -> 6.47 ms, and in the record's longest-first order costs nothing
// (profiles/r03/share_ab.txt).  RTCLJ_STEAL=0: never share.)
// The knobs and the device's slots for policy::choose_split, spp > 1.
static int launch_split(const rt_dscene& ds, const Kernel& v, size_t lds, int n_tiles, const rt_params& p) {
  int forced = 0, slots = 0, rounds = 0;
  if (const char* e = std::getenv("RTCLJ_SPLIT")) {
    forced = std::max(1, std::atoi(e));
  } else {
    slots = launch_slots(ds.device, v.fn, lds, v.t.threads);
    // (28: its pools are the split's answer already; they split only when
    // fewer than RTCLJ_TH4_SPLIT_ROUNDS (1) rounds of them fill the device)
    rounds = v.t.th ? env_int("RTCLJ_TH4_SPLIT_ROUNDS", 1, 1) : env_int("RTCLJ_SPLIT_ROUNDS", 3, 1);
  }
  return policy::choose_split(n_tiles, p.spp, forced, slots, rounds, (p.flags & RT_FLAG_STREAMED) != 0);
}

// the fills a launch needs before its trace kernel, as one launch
static hipError_t enqueue_fills(const FillSet& fills, hipStream_t stream) {
  size_t most = 0;
  for (int k = 0; k < fills.count; ++k) most = std::max(most, fills.n[k]);
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((most + 255) / 256, 2048));
  return enqueue(fill_set_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, fills);
}

// The schedule's sort of n costs: order_kernel (longest-first order, each cost
// halved), and for a plan of U > 0 units plan_kernel behind it.  What
// Schedule::sort_record and rt_schedule_sort enqueue.
static hipError_t enqueue_sort(unsigned* cost, int* order, int n, int U, int smax, int2* units, hipStream_t stream) {
  const hipError_t e = enqueue(order_kernel, dim3(1), dim3(1024), 0, stream, cost, order, n);
  if (e != hipSuccess || U <= 0) return e;
  return enqueue(plan_kernel, dim3(1), dim3(1024), 0, stream, cost, order, n, U, smax, units);
}

// A launch of another shape re-keys the entry: that record was another
// shape's.  Returns whether it did.
bool Schedule::rekey(const ScheduleKey& k) {
  if (std::memcmp(&key, &k, sizeof k) == 0) return false;
  ready = false;
  sort_pending = false;
  key = k;
  return true;
}

// The pending sort of the stream's tile-cost record (sort_pending):
// order_kernel, and plan_kernel for a planned split; the order is ready for
// the next launch of the shape.
int Schedule::sort_record(int n_tiles, int spp) {
  // the next split launch's cost-balanced units, from this record
  const bool plan = sort_plan > 0 && units.cap >= static_cast<size_t>(sort_plan);
  HIP_TRY(enqueue_sort(cost.p, order.p, n_tiles, plan ? sort_plan : 0, std::min(spp, policy::kSplitMax), units.p,
                       stream));
  ready = true;
  sort_pending = false;
  plan_units = plan ? sort_plan : -1;
  return RT_OK;
}

// the split tiles' integer sums: one u64 per channel, added to by the
// splits, converted and zeroed by finalize_kernel
int Schedule::bind_part(KArgs& a, size_t n_elems) {
  bool grew = false;
  HIP_TRY(part.reserve(n_elems, stream, &grew));
  if (grew) {
    HIP_TRY(fill_zero(part, n_elems, stream));
    part_dirty = false;
  }
  if (part_dirty) {   // an earlier launch failed between its trace and finalize kernels
    HIP_TRY(fill_zero(part, part.cap, stream));
    part_dirty = false;
  }
  a.part = part.p;
  return RT_OK;
}

// adaptive schedule: dispatch tiles longest first, by the durations the
// previous launches of this launch shape on this scene and stream measured
// (each launch's added to half the record before it).  split_units: a split
// launch's split units (-1: not split).  *first_order: a shape's first launch
// in a heuristic order.
int Schedule::bind_order(KArgs& a, FillSet& fills, int n_tiles, int spp, int split_units, bool* first_order) {
  bool grew_cost = false, grew_order = false;
  hipError_t e = cost.reserve(n_tiles, stream, &grew_cost);
  if (e == hipSuccess) e = order.reserve(n_tiles, stream, &grew_order);
  if (grew_cost || grew_order || e != hipSuccess) {   // (the record and the order went with the old buffers)
    ready = false;
    sort_pending = false;
  }
  HIP_TRY(e);
  // the previous launch's record, sorted now (stream-ordered after it)
  if (sort_pending)
    if (const int rc = sort_record(n_tiles, spp)) return rc;
  if (ready) {
    a.tile_order = order.p;
  } else if (env_int("RTCLJ_FIRST_ORDER", 1, 0) == 1) {
    // No record yet: the tiles bottom-up.  The reference's scenes (and
    // C1-C4) put the ground and its bodies below the sky: the expensive
    // tiles start first and the launch ends on sky tiles, where row-major
    // order ended on the ground's.  C1's first frame of a shape 5.13-5.19
    // ms against 5.25 row-major (tools/first_frame.py, 9 pairs, two
    // rounds; profiles/r06/first_order/); RTCLJ_FIRST_ORDER=0: row-major.
    // Tile sharing still balances the tail, as in plain order.
    HIP_TRY(enqueue(iota_rev_kernel, dim3(static_cast<unsigned>((n_tiles + 255) / 256)), dim3(256), 0, stream, order.p,
                    n_tiles));
    a.tile_order = order.p;
    *first_order = true;
  }
  a.tile_cost = cost.p;
  // a split launch in the recorded order: with RTCLJ_SPLIT_PLAN=1, the
  // cost-balanced units the previous launch of the shape planned (when it
  // planned this many).  Off by default: C1's 8-GPU shard 1.10-1.15 ms
  // against 0.99-1.02 with uniform splits, the 4-GPU one 1.93 vs 1.69
  // (profiles/r04/split_plan/; round 2's cost-sized splits lost the same
  // way): a heavy tile's many short pools each end with idle lanes.
  if (split_units >= 0 && ready && plan_units == split_units && env_int("RTCLJ_SPLIT_PLAN", 0, 0) != 0)
    a.unit_tab = units.p;
  // the costs decay (order_kernel halves them after sorting): zeroed only
  // when this launch shape starts a new history
  if (!ready) fills.add(cost.p, 0, n_tiles * sizeof(unsigned));
  return RT_OK;
}

// Tile sharing for a launch of whole tiles: the stream's words, counts, sums
// and owner table bound to the arguments, this launch's epoch, and the
// helpers added to *grid (the units, then the thieves, dispatched last, i.e.
// as the units' slots free up in the launch's tail).  slots: the workgroups
// the device holds at once (>= 1).
// Tile sharing, A/B knobs read at every launch:
// RTCLJ_STEAL=0 (off: the static sample split for launches of few tiles, as
// before), RTCLJ_THIEVES (helper workgroups per workgroup slot of the
// device), RTCLJ_STEAL_MIN (unclaimed samples a tile needs for a helper to join)
int Schedule::bind_sharing(KArgs& a, FillSet& fills, int n_tiles, int n_units, int slots, bool new_shape,
                           bool first_order, int64_t* grid) {
  const int n_owner = 2 * slots;   // owner entries: twice the resident workgroups
  // (at most 32 per slot: a tile's helper count stays below 2^16)
  *grid += static_cast<int64_t>(std::min(32, env_int("RTCLJ_THIEVES", 4, 0))) * slots;
  if (*grid > INT_MAX) *grid = n_units;
  if (!stealc) {
    HIP_TRY(stealc.alloc(2));
    HIP_TRY(fill_zero(stealc, 2, stream));
  }
  const size_t nsum = static_cast<size_t>(n_tiles) * kPoolPx * 3;
  bool grew[3] = {false, false, false};
  hipError_t e = word.reserve(n_tiles, stream, &grew[0]);
  if (e == hipSuccess) e = done.reserve(n_tiles, stream, &grew[1]);
  if (e == hipSuccess) e = sum.reserve(nsum, stream, &grew[2]);
  HIP_TRY(e);   // (one that failed is empty, and grows again at the next launch)
  if (grew[0] || grew[1] || grew[2]) {
    // words 0: lo = hi, nothing to steal until an owner publishes; sums
    // and done counts 0 (the kernel keeps them so between uses)
    HIP_TRY(fill_zero(word, n_tiles, stream));
    HIP_TRY(fill_zero(done, n_tiles, stream));
    HIP_TRY(fill_zero(sum, nsum, stream));
    new_shape = true;
  }
  bool grew_owner = false;
  HIP_TRY(owner.resize(n_owner, stream, &grew_owner));
  if (grew_owner) new_shape = true;
  if (!epoch_started) {   // (RTCLJ_EPOCH_START: tests start a stream near the wrap)
    epoch = static_cast<unsigned>(std::min(0xffff, env_int("RTCLJ_EPOCH_START", 1, 1)) - 1);
    epoch_started = true;
  }
  epoch = (epoch + 1) & 0xffffu;
  if (epoch == 0) {   // wrapped: no word or owner entry may carry the epoch's last use
    epoch = 1;
    new_shape = true;
  }
  a.epoch = epoch;
  // a new shape (or a wrap): no tile is being run, and no word holds this
  // launch's epoch.  (Old owner entries would only name words of other
  // epochs, but tile indices of another shape may exceed this one's; a word
  // last published 65,535 launches ago carries the epoch a wrap reuses.)
  if (new_shape) {
    fills.add(owner.p, 0xff, n_owner * sizeof(int));
    fills.add(word.p, 0, n_tiles * sizeof(unsigned long long));
  }
  // owners publish only in the launch's last RTCLJ_SHARE_ROUNDS rounds of
  // units (default 2; a round = the workgroups the device holds at once.
  // C4 plain order: WRITE_SIZE 2.90 GB per launch at every round, 0.44 at
  // 2, 0.60 at 3; C1's timing the same at 1, 2, 3 or every round:
  // profiles/r04/share_rounds/)
  a.share_from = static_cast<int>(std::max<int64_t>(
      0, n_units - static_cast<int64_t>(env_int("RTCLJ_SHARE_ROUNDS", 2, 0)) * slots));
  a.word = word.p;
  a.done = done.p;
  a.sum = sum.p;
  a.owner = owner.p;
  a.n_owner = n_owner;
  a.stealc = stealc.p;
  a.steal_min = env_int("RTCLJ_STEAL_MIN", 256, 1);
  // claims of up to 1024 samples in the record's longest-first order (the
  // heavy tiles start first: fewer claims, 6.03 -> 6.00 ms on C1); in plain
  // order up to 1/48 of the tile's pool (0: the kernel's per-pool rule; C1's
  // 6,400: 128 -- helpers then need small claims to balance the tail;
  // C4's 64,000: 1024)
  a.batch_max = env_int("RTCLJ_BATCH_MAX", (a.tile_order && !first_order) ? 1024 : 0, 0);
  return RT_OK;
}

// Path export for split launches (KArgs xq; RTCLJ_EXPORT=1, A/B): a wave
// whose batches are spent and which holds at most RTCLJ_EXPORT_LIM paths
// (default 64: as soon as its batches are spent) writes them out and
// leaves, so a unit's workgroup frees its slot without draining; the sweep
// launch runs the records.  At most one record per thread of a unit.
int Schedule::bind_export(KArgs& a, FillSet& fills, size_t records) {
  HIP_TRY(xq.reserve(records * 4, stream));
  if (!xq_n) HIP_TRY(xq_n.alloc(2));
  fills.add(xq_n.p, 0, 2 * sizeof(unsigned));
  a.xq = xq.p;
  a.xq_n = xq_n.p;
  a.compact = std::min(64, env_int("RTCLJ_EXPORT_LIM", 64, 1));
  ++xq_launches;
  return RT_OK;
}

// Behind a launch that recorded its tiles' costs: this record's sort, at the
// next launch of the shape on the stream (RTCLJ_SORT_EAGER=1, A/B: right
// behind this launch, as before round 6; within noise on every bench.py leg,
// profiles/r06/sort_ab/).  plan_units_next: the units of a wholly split
// launch, for which RTCLJ_SPLIT_PLAN=1 plans the next one (-1: none).
int Schedule::record(int n_tiles, int spp, int plan_units_next) {
  sort_pending = true;
  ready = false;
  sort_plan = -1;
  if (plan_units_next >= 0 && env_int("RTCLJ_SPLIT_PLAN", 0, 0) != 0) {
    HIP_TRY(units.reserve(plan_units_next, stream));
    sort_plan = plan_units_next;
  }
  if (env_int("RTCLJ_SORT_EAGER", 0, 0) != 0) return sort_record(n_tiles, spp);
  return RT_OK;
}

// rt_launch, and rt_launch_accum's pass (acc_sums: the accumulator's
// [rows][width][3] sums; d_out NULL).  A pass is the launch with no whole
// tiles (n_whole = 0: every unit, one per tile or `split` per tile, adds its
// integer sums to part[] = acc_sums by atomics) and no finalize_kernel behind
// it; the stream's own part buffer and its part_dirty flag are left alone.
// rt_adapt_step's pass adds `active`, a device list of n_active tiles: the
// launch's tile order, whose length stands for the tile count in the split and
// the unit count -- the same launch with a shorter order.  It needs 8 x 8
// tiles, and neither reads nor writes the stream's record (no cost, no order).
// rt_budget_trace_fused's pass gives `units` instead, a device table of n_tab
// explicit units (KArgs::unit_tab: a tile and one of s sample ranges of p->spp
// each; budget.h makes it): one workgroup per entry and no split of its own,
// under the same conditions as `active` (which it excludes); it needs acc_sums.
int rtclj::launch_impl(const rt_dscene* ds, const rt_camera* c, const rt_params* p, float* d_out, uint64_t* d_counters,
                       void* hip_stream, unsigned long long* acc_sums, const char* who, const int* active,
                       int n_active, const int2* units, int n_tab) {
  if (!ds || !c || !p || (!d_out && !acc_sums)) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  if (const int rc = check_frame_args(who, *p)) return rc;
  const int rows = rows_out(*p);
  if (rows < 0) return set_error(RT_E_ARG, std::string(who) + ": bad row selection");
  if (rows == 0) return RT_OK;
  HIP_TRY(hipSetDevice(ds->device));
  KArgs a{};
  a.geo = ds->geo;
  a.geo2 = reinterpret_cast<const Pair*>(ds->geo2);
  a.sph = ds->sph;
  a.mat = ds->mat;
  a.kind = ds->kind;
  a.out = d_out;
  a.counters = reinterpret_cast<unsigned long long*>(d_counters);
  pack_frame(a, *c, *p, rows);
  a.n = ds->n;
  a.n_pad = ds->n_pad;
  a.max_depth = p->max_depth;
  a.realm = (p->flags & RT_FLAG_REALM) ? 1 : 0;
  Kernel v;
  if (const int rc = bind_variant(who, *ds, *p, a, &v)) return rc;
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int th = policy::variant_rows(v.t);   // the variant's tile rows
  const int gx = (p->width + kTile - 1) / kTile, gy = (rows + th - 1) / th;
  if (active && (th != kTile || n_active <= 0 || n_active > gx * gy))
    return set_error(RT_E_ARG, std::string(who) + ": variant " + std::to_string(v.vsel) + " has no 8 x 8 tiles");
  if (units && th != kTile)
    return set_error(RT_E_ARG, std::string(who) + ": variant " + std::to_string(v.vsel) + " has no 8 x 8 tiles");
  if (units && (active || !acc_sums || n_tab <= 0))
    return set_error(RT_E_ARG, std::string(who) + ": a unit table needs an accumulator, no tile list and n_units > 0");
  const int n_tiles = active ? n_active : gx * gy;
  a.tiles_x = gx;
  if (const int rc = bind_debug(ds->device, v, a)) return rc;
  size_t lds = 0;
  if (const int rc = bind_lds(*ds, v, &lds)) return rc;
  // the stream's entry: adaptive schedule and split partial sums
  Schedule* sch = nullptr;
  std::unique_lock<std::mutex> sched_lock;
  if (!active && !units) {
    sched_lock = std::unique_lock<std::mutex>(ds->sched.mu);
    sch = ds->sched.entry(stream);
  }
  const bool steal = sch && env_int("RTCLJ_STEAL", 1, 0) != 0 && !v.t.stats && v.t.walk != policy::WALK_SORTED;
  // (a unit table is the split already)
  const int split = ((sch || acc_sums) && p->spp > 1 && !units) ? launch_split(*ds, v, lds, n_tiles, *p) : 1;
  // (an accumulating pass: every unit's sums go to part[])
  const int n_whole = (split > 1 || acc_sums) ? 0 : n_tiles;
  a.split = split;
  a.n_whole = n_whole;
  a.rt_magic = magic64(a.row_tile);
  const int64_t n_units64 = units ? n_tab : n_whole + static_cast<int64_t>(n_tiles - n_whole) * split;
  if (n_units64 > INT_MAX) return set_error(RT_E_ARG, std::string(who) + ": frame too large");
  const int n_units = static_cast<int>(n_units64);
  const bool finalize = split > 1 && !acc_sums;   // the split tiles' sums go through the stream's part buffer
  if (acc_sums) a.part = acc_sums;
  else if (finalize)
    if (const int rc = sch->bind_part(a, static_cast<size_t>(rows) * p->width * 3)) return rc;
  const bool new_shape =
      sch && sch->rekey(ScheduleKey{a.width, a.rows_out, a.row_begin, a.row_tile, a.tile_first, a.tile_step, gx, gy});
  FillSet fills;
  bool first_order = false;
  if (sch && g_schedule.load() == 0)
    if (const int rc = sch->bind_order(a, fills, n_tiles, p->spp, split > 1 ? n_units - n_whole : -1, &first_order))
      return rc;
  if (active) a.tile_order = active;
  if (units) {
    a.unit_tab = units;
    a.tile_order = nullptr;
  }
  int64_t grid = n_units;
  // Sharing balances a launch whose tiles have no cost record (plain order:
  // a process's or a shape's first frame).  In the recorded longest-first
  // order the cheap tiles come last and the tail is short without it (C1
  // 5.94 ms either way), while its claims and helpers' scans are HBM atomics
  // (C1: 31 vs 11 MB per launch; profiles/r04/share_rounds/): off there
  // unless RTCLJ_SHARE_RECORDED=1.
  if (steal && split == 1 && !acc_sums && (!a.tile_order || first_order || env_int("RTCLJ_SHARE_RECORDED", 0, 0) != 0)) {
    const int slots = std::max(1, launch_slots(ds->device, v.fn, lds, v.t.threads));
    if (const int rc = sch->bind_sharing(a, fills, n_tiles, n_units, slots, new_shape, first_order, &grid)) return rc;
  }
  a.n_units = n_units;
  // a wave's claims on an unshared pool: guided (an eighth of what is left
  // past its last batch), 64 .. RTCLJ_LDS_BATCH (default 256; fixed 64-index
  // batches were round 3's: C1 5.960 -> 5.916 ms, C2 287.9 -> 286.1 ms,
  // profiles/r04/lds_batch/)
  a.lds_batch_max = std::max(64, env_int("RTCLJ_LDS_BATCH", 256, 64));
  const bool xport = sch && split > 1 && v.sweep && env_int("RTCLJ_EXPORT", 0, 0) != 0;
  if (xport)
    if (const int rc = sch->bind_export(a, fills, static_cast<size_t>(n_units) * v.t.threads)) return rc;

  if (fills.count) HIP_TRY(enqueue_fills(fills, stream));
  const dim3 block(v.t.threads);
  if (finalize) sch->part_dirty = true;   // (cleared once finalize_kernel is enqueued)
  HIP_TRY(enqueue(v.fn, dim3(static_cast<unsigned>(grid)), block, lds, stream, a));
  if (xport) {
    // the sweep: one workgroup per slot the device holds, each starting on
    // its own 256 records and claiming more; a workgroup past the records
    // leaves at once.  It adds into part[], so it runs before finalize_kernel.
    KArgs b = a;
    b.word = nullptr;
    b.tile_cost = nullptr;
    b.tile_order = nullptr;
    b.unit_tab = nullptr;
    b.compact = is_bvh_scan(v.t.scan) ? std::min(b.mb_paths, env_int("RTCLJ_COMPACT", b.mb_paths, 0)) : 0;
    const int sw = std::max(1, launch_slots(ds->device, v.sweep, lds, v.t.threads));
    HIP_TRY(enqueue(v.sweep, dim3(static_cast<unsigned>(sw)), block, lds, stream, b));
  }
  if (finalize) {
    HIP_TRY(enqueue(finalize_kernel, dim3(n_tiles - n_whole), dim3(kTile * 3 * th), 0, stream, a.part, a.tile_order,
                    n_whole, gx, th, p->width, rows, d_out, p->spp, a.realm));
    sch->part_dirty = false;
  }
  if (a.tile_cost)
    if (const int rc = sch->record(n_tiles, p->spp, (split > 1 && n_whole == 0) ? n_units : -1)) return rc;
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

extern "C" int rt_launch(const rt_dscene* ds, const rt_camera* c, const rt_params* p, float* d_out,
                         uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!d_out) return set_error(RT_E_ARG, "rt_launch: NULL argument");
  return launch_impl(ds, c, p, d_out, d_counters, hip_stream, nullptr);
}

// A device's start-up ahead of the first render (rt.h): the context, the
// kernels' code object (loaded for the device on a function lookup), the NULL
// stream's first work (its hardware queue) and a small pageable D2H copy (the
// runtime's staging for pageable transfers, which the first frame's gather
// otherwise pays).  Each part timed on the host.
extern "C" int rt_prepare(int device, double* out_ms4) {
  clear_error();
  using Clk = std::chrono::steady_clock;
  auto ms = [](Clk::time_point a, Clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return set_error(RT_E_NODEV, "rt_prepare: device " + std::to_string(device) + " not available");
  const auto t0 = Clk::now();
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipFree(nullptr));
  const auto t1 = Clk::now();
  hipFuncAttributes fa{};
  HIP_TRY(hipFuncGetAttributes(&fa, variant_fn(policy::kFull4)));
  const auto t2 = Clk::now();
  constexpr size_t kProbe = 64 * 1024;
  DevBuf<uint32_t> d;
  HIP_TRY(d.alloc(kProbe / 4));
  hipError_t e = fill_zero(d, kProbe / 4, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  const auto t3 = Clk::now();
  std::vector<unsigned char> host(kProbe);
  if (e == hipSuccess) e = hipMemcpy(host.data(), d.p, kProbe, hipMemcpyDeviceToHost);
  const auto t4 = Clk::now();
  if (e != hipSuccess) return hip_fail(e, "rt_prepare");
  if (out_ms4) {
    out_ms4[0] = ms(t0, t1);
    out_ms4[1] = ms(t1, t2);
    out_ms4[2] = ms(t2, t3);
    out_ms4[3] = ms(t3, t4);
  }
  return RT_OK;
}

// Stats builds read-back: sums and clears the kDbg debug counters of every
// device that ran a stats launch; the first n of them go to out.
static int debug_stats(uint64_t* out, int n, const char* who) {
  clear_error();
  if (!out || n < 0 || n > kDbg) return set_error(RT_E_ARG, std::string(who) + ": NULL, or a count outside 0 .. 40");
  for (int i = 0; i < n; ++i) out[i] = 0;
  std::lock_guard<std::mutex> lk(g_dbg_mu);
  for (int d = 0; d < kDbgDevices; ++d) {
    if (!g_dbg[d]) continue;
    uint64_t v[kDbg];
    HIP_TRY(hipSetDevice(d));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(v, g_dbg[d], sizeof v, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(g_dbg[d], 0, sizeof v));
    for (int i = 0; i < n; ++i) out[i] += v[i];
  }
  return RT_OK;
}
extern "C" int rt_debug_stats(uint64_t* out32) { return debug_stats(out32, 32, "rt_debug_stats"); }
extern "C" int rt_debug_stats_ext(uint64_t* out, int n) { return debug_stats(out, n, "rt_debug_stats_ext"); }

// Steals of the launches on (ds, stream) since the last call: out2 =
// {steals, samples stolen}; waits for the stream, then clears them.
extern "C" int rt_steal_stats(const rt_dscene* ds, void* hip_stream, uint64_t* out2) {
  clear_error();
  if (!ds || !out2) return set_error(RT_E_ARG, "rt_steal_stats: NULL argument");
  out2[0] = out2[1] = 0;
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  std::lock_guard<std::mutex> lk(ds->sched.mu);
  const Schedule* e = ds->sched.find(stream);
  if (!e || !e->stealc) return RT_OK;
  HIP_TRY(hipSetDevice(ds->device));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(out2, e->stealc.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(e->stealc.p, 0, 2 * sizeof(uint64_t)));
  return RT_OK;
}

// Path export of the split launches on (ds, stream) (diagnostic): out2 =
// {export launches since the last call, records the latest one wrote}; waits
// for the stream.
extern "C" int rt_export_stats(const rt_dscene* ds, void* hip_stream, uint64_t* out2) {
  clear_error();
  if (!ds || !out2) return set_error(RT_E_ARG, "rt_export_stats: NULL argument");
  out2[0] = out2[1] = 0;
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  std::lock_guard<std::mutex> lk(ds->sched.mu);
  Schedule* e = ds->sched.find(stream);
  if (!e || !e->xq_n) return RT_OK;
  HIP_TRY(hipSetDevice(ds->device));
  HIP_TRY(hipStreamSynchronize(stream));
  unsigned n[2] = {0, 0};
  HIP_TRY(hipMemcpy(n, e->xq_n.p, sizeof n, hipMemcpyDeviceToHost));
  out2[0] = e->xq_launches;
  out2[1] = n[0];
  e->xq_launches = 0;
  return RT_OK;
}

// The adaptive schedule's entry of (ds, stream), read out (diagnostic): waits
// for the stream, then copies the per-tile costs, the order as it stands and
// the planned units.  Changes nothing: a pending sort stays pending.
extern "C" int rt_schedule_read(const rt_dscene* ds, void* hip_stream, rt_schedule_info* info, uint32_t* host_cost,
                                int32_t* host_order, int32_t* host_units, int cap_tiles, int cap_units) {
  clear_error();
  if (cap_tiles < 0 || cap_units < 0 || ((host_cost || host_order) && cap_tiles == 0) || (host_units && cap_units == 0))
    return set_error(RT_E_ARG, "rt_schedule_read: a buffer's cap is too small");
  if (!ds || !info) return set_error(RT_E_ARG, "rt_schedule_read: NULL argument");
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  std::lock_guard<std::mutex> lk(ds->sched.mu);
  const Schedule* e = ds->sched.find(stream);
  rt_schedule_info out{};
  out.plan_units = out.sort_plan = -1;
  out.max_streams = kSchedStreams;
  if (!e) {
    *info = out;
    return RT_OK;
  }
  const int n = e->key.gx * e->key.gy;
  out.exists = 1;
  out.n_tiles = n;
  out.ready = e->ready ? 1 : 0;
  out.sort_pending = e->sort_pending ? 1 : 0;
  out.plan_units = e->plan_units;
  out.sort_plan = e->sort_plan;
  out.has_record = (n > 0 && e->cost.cap >= static_cast<size_t>(n) && e->order.cap >= static_cast<size_t>(n)) ? 1 : 0;
  const int n_rec = out.has_record ? n : 0;
  const int n_units = (e->plan_units > 0 && e->units.cap >= static_cast<size_t>(e->plan_units)) ? e->plan_units : 0;
  if ((host_cost || host_order) && n_rec > cap_tiles)
    return set_error(RT_E_ARG, "rt_schedule_read: cap_tiles " + std::to_string(cap_tiles) + " < " +
                                   std::to_string(n_rec) + " tiles");
  if (host_units && n_units > cap_units)
    return set_error(RT_E_ARG, "rt_schedule_read: cap_units " + std::to_string(cap_units) + " < " +
                                   std::to_string(n_units) + " units");
  HIP_TRY(hipSetDevice(ds->device));
  HIP_TRY(hipStreamSynchronize(stream));
  if (host_cost && n_rec) HIP_TRY(hipMemcpy(host_cost, e->cost.p, n_rec * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (host_order && n_rec) HIP_TRY(hipMemcpy(host_order, e->order.p, n_rec * sizeof(int), hipMemcpyDeviceToHost));
  if (host_units && n_units) HIP_TRY(hipMemcpy(host_units, e->units.p, n_units * sizeof(int2), hipMemcpyDeviceToHost));
  *info = out;
  return RT_OK;
}

// The schedule's sort on the caller's data (diagnostic; no scene): n costs
// and the order's and units' initial contents go up, enqueue_sort runs on
// hip_stream as Schedule::sort_record runs it, and the halved costs, the order
// and the U units come back.
extern "C" int rt_schedule_sort(int device, uint32_t* host_cost_inout, int n, int32_t* host_order, int U, int smax,
                                int32_t* host_units, void* hip_stream) {
  clear_error();
  if (!host_cost_inout || !host_order || (U > 0 && !host_units))
    return set_error(RT_E_ARG, "rt_schedule_sort: NULL argument");
  if (n <= 0) return set_error(RT_E_ARG, "rt_schedule_sort: n must be positive");
  if (U < 0 || (U != 0 && U < n)) return set_error(RT_E_ARG, "rt_schedule_sort: U must be 0 or at least n");
  if (smax < 1 || smax > policy::kSplitMax)
    return set_error(RT_E_ARG, "rt_schedule_sort: smax must be 1 .. " + std::to_string(policy::kSplitMax));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return set_error(RT_E_NODEV, "rt_schedule_sort: device " + std::to_string(device) + " not available");
  HIP_TRY(hipSetDevice(device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  DevBuf<unsigned> cost;
  DevBuf<int> order;
  DevBuf<int2> units;
  HIP_TRY(cost.alloc(n));
  HIP_TRY(order.alloc(n));
  if (U > 0) HIP_TRY(units.alloc(U));
  const size_t nb = static_cast<size_t>(n) * 4, ub = static_cast<size_t>(U) * sizeof(int2);
  HIP_TRY(hipMemcpy(cost.p, host_cost_inout, nb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(order.p, host_order, nb, hipMemcpyHostToDevice));
  if (U > 0) HIP_TRY(hipMemcpy(units.p, host_units, ub, hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());   // (the copies have landed before hip_stream's kernels start)
  HIP_TRY(enqueue_sort(cost.p, order.p, n, U, smax, units.p, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(host_cost_inout, cost.p, nb, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(host_order, order.p, nb, hipMemcpyDeviceToHost));
  if (U > 0) HIP_TRY(hipMemcpy(host_units, units.p, ub, hipMemcpyDeviceToHost));
  return RT_OK;
}

// Stats build wave timeline of `device`: up to n waves x {t_start, t_end,
// hw_id, xcc_id} (s_memrealtime ticks, 100 MHz); cleared after the copy.
extern "C" int rt_debug_waves(int device, uint64_t* out, size_t n_waves) {
  clear_error();
  if (!out) return set_error(RT_E_ARG, "rt_debug_waves: NULL");
  if (device < 0 || device >= kDbgDevices) return set_error(RT_E_ARG, "rt_debug_waves: bad device");
  std::lock_guard<std::mutex> lk(g_dbg_mu);
  if (!g_dbgw[device]) return 0;
  if (n_waves > kDbgWaves) n_waves = kDbgWaves;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, g_dbgw[device], 4 * n_waves * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(g_dbgw[device], 0, 4 * kDbgWaves * sizeof(uint64_t)));
  return static_cast<int>(n_waves);
}
