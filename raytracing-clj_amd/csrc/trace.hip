// trace.hip — the product library's gfx950 code object and host side: the
// shipped kernel's instantiations (trace_kernel.h: the default BVH walk in its
// two LDS images and its fallbacks), the schedule / split / quantise / fill
// kernels, the accumulator's resolve / add kernels, the adaptive sampler's
// evaluation / resolve kernels, and rt_scene_upload / rt_launch /
// rt_launch_accum / rt_adapt_step and the rt_accum and rt_adapt entries.  The A/B scans, the
// direction-coherent waves and the statistics builds live in trace_diag.hip
// (librtclj_diag.so only).  DESIGN.md §3.  The first-hit feature pass
// (first_hit.h: feat_kernel, feat_resolve_kernel) and the rt_feat entries are
// here too.
#include "trace_kernel.h"
#define RT_FIRST_HIT_KERNEL
#include "first_hit.h"

#include <algorithm>
#include <chrono>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

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
struct QThr {
  float t[256];
};
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

// rt_accum_resolve / rt_accum_resolve_u8: an accumulator's integer sums as a
// frame, by finalize_kernel's conversion -- RN(float(sum)) * 2^-24, / nf
// (realm: * (1/nf)), nf = RN(float(samples per pixel)) -- and, for the bytes,
// quantize_kernel's threshold search on that float, in one pass: a thread
// reads two sums as 16 bytes and writes the floats (out_f) and / or the bytes
// (out_u8) of both; an odd count's last sum is thread 0's.  The sums are only
// read: the host shows the frame and goes on adding passes.
__global__ __launch_bounds__(256) void resolve_kernel(const unsigned long long* __restrict__ sums, size_t n, float nf,
                                                       int realm, float* __restrict__ out_f,
                                                       uint8_t* __restrict__ out_u8, const QThr q) {
  __shared__ float s_t[256];
  if (out_u8) {   // (uniform)
    s_t[threadIdx.x] = q.t[threadIdx.x];
    __syncthreads();
  }
  auto put = [&](size_t i, unsigned long long sum) {
    const float tot = static_cast<float>(sum) * 0x1p-24f;
    const float c = realm ? tot * (1.0f / nf) : tot / nf;
    if (out_f) out_f[i] = c;
    if (out_u8) {
      int b = 0;
#pragma unroll
      for (int step = 128; step > 0; step >>= 1)
        if (s_t[b + step] <= c) b += step;   // b + step <= 255
      out_u8[i] = static_cast<uint8_t>(b);
    }
  };
  const ulonglong2* __restrict__ s2 = reinterpret_cast<const ulonglong2*>(sums);   // (hipMalloc's alignment)
  const size_t pairs = n / 2, stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < pairs; i += stride) {
    const ulonglong2 v = s2[i];
    put(2 * i, v.x);
    put(2 * i + 1, v.y);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) put(n - 1, sums[n - 1]);
}

// rt_accum_add: another accumulator's sums (staged in HBM) added to this
// one's, by the atomics the trace kernel's units use, so that a pass running
// on another stream may add to the same words.
__global__ __launch_bounds__(256) void accum_add_kernel(unsigned long long* __restrict__ sums,
                                                         const unsigned long long* __restrict__ add, size_t n) {
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
    const unsigned long long v = add[i];
    if (v) __hip_atomic_fetch_add(&sums[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Adaptive sampling (rt_adapt, rt.h): the stopping rule over the two halves'
// integer sums, for the tiles of the active list -- one wave per 8 x 8 tile,
// one lane per pixel (row lane / 8, column lane % 8; a ragged tile's lanes
// outside the frame hold nothing).  A lane reads its pixel's three u64 of
// each half as a 16-byte and an 8-byte load (a pixel is 24 bytes: the pair
// comes first where the pixel starts on 16 bytes, last where it does not),
// adds D = sum |h0 - h1| and S = sum (h0 + h1) over its channels, and the
// wave adds the lanes' by shuffles: 192 terms below 2^56 each, below 2^64 in
// all.  Lane 0 then holds the tile's rule, D * 2^16 <= tol * S as 128-bit
// integers (the high halves by shift and __umul64hi), writes the tile's count
// and, when the tile goes on, appends it to the next list: a position from an
// atomic on state[0], the tile's pixels added to state[1].  The order of the
// next list is whatever the atomics give: no bit depends on it.  decide = 0
// (a step after which no tile is tested): the counts only.  Block 0 zeroes
// `state_next`, the pair the evaluation after this one counts in (the host
// has read it back before this kernel was enqueued).
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), off);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), off);
    v += (static_cast<unsigned long long>(hi) << 32) | lo;
  }
  return v;
}
// a pixel's three sums at s[0..2], s = sums + e (e: the element index, whose
// parity is the 16-byte alignment: hipMalloc's base is aligned)
__device__ __forceinline__ void load_px3(const unsigned long long* __restrict__ s, bool even,
                                         unsigned long long (&v)[3]) {
  if (even) {
    const ulonglong2 p = *reinterpret_cast<const ulonglong2*>(s);
    v[0] = p.x;
    v[1] = p.y;
    v[2] = s[2];
  } else {
    const ulonglong2 p = *reinterpret_cast<const ulonglong2*>(s + 1);
    v[0] = s[0];
    v[1] = p.x;
    v[2] = p.y;
  }
}
constexpr int kEvalWaves = 4;   // tiles per block of adapt_eval_kernel
__global__ __launch_bounds__(64 * kEvalWaves) void adapt_eval_kernel(
    const unsigned long long* __restrict__ h0, const unsigned long long* __restrict__ h1, int width, int rows,
    int tiles_x, const int* __restrict__ active, int n_active, int* __restrict__ next, unsigned* __restrict__ state,
    unsigned* __restrict__ state_next, uint32_t* __restrict__ counts, uint32_t count, uint32_t tol_q16, int decide) {
  if (state_next && blockIdx.x == 0 && threadIdx.x < 2) state_next[threadIdx.x] = 0u;
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int pos = static_cast<int>(blockIdx.x) * kEvalWaves + (static_cast<int>(threadIdx.x) >> 6);
  if (pos >= n_active) return;   // (the whole wave)
  const int tile = active[pos];
  if (!decide) {
    if (lane == 0) counts[tile] = count;
    return;
  }
  const int tby = tile / tiles_x, tbx = tile - tby * tiles_x;
  const int x = tbx * kTile + (lane & 7), y = tby * kTile + (lane >> 3);
  unsigned long long d = 0ull, s = 0ull;
  if (x < width && y < rows) {
    const size_t px = static_cast<size_t>(y) * width + x;
    unsigned long long a[3], b[3];
    load_px3(h0 + px * 3, (px & 1) == 0, a);
    load_px3(h1 + px * 3, (px & 1) == 0, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      d += a[c] > b[c] ? a[c] - b[c] : b[c] - a[c];
      s += a[c] + b[c];
    }
  }
  d = wave_sum_u64(d);
  s = wave_sum_u64(s);
  if (lane == 0) {
    // D * 2^16 against tol * S, both as (high, low) u64 pairs
    const unsigned long long l_hi = d >> 48, l_lo = d << 16;
    const unsigned long long r_hi = __umul64hi(static_cast<unsigned long long>(tol_q16), s);
    const unsigned long long r_lo = static_cast<unsigned long long>(tol_q16) * s;
    const bool converged = l_hi < r_hi || (l_hi == r_hi && l_lo <= r_lo);
    counts[tile] = count;
    if (!converged) {
      const int vw = min(kTile, width - tbx * kTile), vh = min(kTile, rows - tby * kTile);
      const unsigned at = __hip_atomic_fetch_add(&state[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      next[at] = tile;
      __hip_atomic_fetch_add(&state[1], static_cast<unsigned>(vw * vh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// rt_adapt_resolve / rt_adapt_resolve_u8: resolve_kernel's conversion of
// h0 + h1 with the count of the element's own tile.  Block row y is frame row
// y; a thread reads two sums of each half as 16 bytes (the row's first
// element alone where the row starts off 16 bytes: `head`), thread 0 of the
// row's first block the head and the odd tail.
__global__ __launch_bounds__(256) void adapt_resolve_kernel(const unsigned long long* __restrict__ h0,
                                                             const unsigned long long* __restrict__ h1,
                                                             const uint32_t* __restrict__ counts, int width,
                                                             int tiles_x, int realm, float* __restrict__ out_f,
                                                             uint8_t* __restrict__ out_u8, const QThr q) {
  __shared__ float s_t[256];
  if (out_u8) {   // (uniform)
    s_t[threadIdx.x] = q.t[threadIdx.x];
    __syncthreads();
  }
  const int y = static_cast<int>(blockIdx.y), w3 = width * 3;
  const size_t e0 = static_cast<size_t>(y) * w3;
  const uint32_t* __restrict__ crow = counts + static_cast<size_t>(y / kTile) * tiles_x;
  auto put = [&](int c, unsigned long long sum) {
    const uint32_t n = crow[(c / 3) / kTile];
    const float nf = static_cast<float>(n > 0u ? n : 1u);   // RN(float(count))
    const float tot = static_cast<float>(sum) * 0x1p-24f;
    const float v = realm ? tot * (1.0f / nf) : tot / nf;
    if (out_f) out_f[e0 + c] = v;
    if (out_u8) {
      int b = 0;
#pragma unroll
      for (int step = 128; step > 0; step >>= 1)
        if (s_t[b + step] <= v) b += step;   // b + step <= 255
      out_u8[e0 + c] = static_cast<uint8_t>(b);
    }
  };
  const int head = static_cast<int>(e0 & 1), pairs = (w3 - head) / 2;
  const int stride = static_cast<int>(gridDim.x) * 256;
  for (int j = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x); j < pairs; j += stride) {
    const int c = head + 2 * j;
    const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(h0 + e0 + c);
    const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(h1 + e0 + c);
    put(c, a.x + b.x);
    put(c + 1, a.y + b.y);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head) put(0, h0[e0] + h1[e0]);
    if ((w3 - head) & 1) put(w3 - 1, h0[e0 + w3 - 1] + h1[e0 + w3 - 1]);
  }
}

// The first active list: every tile, bottom-up as iota_rev_kernel's first
// order (the expensive ground tiles first), and the counts' zeroing.
__global__ __launch_bounds__(256) void adapt_reset_kernel(int* __restrict__ list, uint32_t* __restrict__ counts,
                                                           unsigned* __restrict__ state, int n) {
  const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (i < n) {
    list[i] = n - 1 - i;
    counts[i] = 0u;
  }
  if (i < 4) state[i] = 0u;
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
// Kernel variants (rt_set_variant).  The product library carries the default
// traversal and its fallbacks:
//   22 BVH in LDS, 4-body leaves, compact image (u8 node-index stack, u32
//      pixel sums with counted wraps, 8-byte pixel table): seven workgroups
//      per CU -- the default where spp < 65536, albedos lie in [-1, 1], the
//      tree has <= 256 nodes and the frame is at most 65536 pixels wide and high
//   16 the same walk in the full image (u16 stack of node addresses, u64 sums)
//   26 22's compact image in 16-wave workgroups (one tree image per 16
//      waves, 64 VGPRs: 8 waves per SIMD): the default for scenes whose
//      4-body image is too big for 22 (C4), where 22 applies and two fit a CU
//   24 the same in 8-wave workgroups: where three of those fit and not two of 26's
//   28 22 on 8 x 4-pixel pools (whole pools for launches of few 8 x 8 tiles
//      instead of sample splits: measured slower, selected only explicitly
//      or by RTCLJ_TH4)
//   18 BVH in LDS, 8-body leaves (large scenes where 24 does not fit)
//   12 BVH (2-body leaves) read from global memory: a tree too big for LDS
//    5 linear scan, grouped, table through the scalar cache: a tree too deep
//    0 = default (22 where it applies, else 16; 26, 24, else 18, when the 4-body tree's LDS image is large)
// The diagnostic library (lib/librtclj_diag.so) adds, from trace_diag.hip, the
// A/B variants -- 1, 2 simple scan (LDS, scalar cache), 4 grouped scan in LDS
// (north_star's LDS-staged scan), 8, 9 packed pairs, 11 BVH with 2-body leaves
// in LDS, 20 / 21 direction-coherent waves (sorted_kernel) -- and the
// statistics builds 3, 6, 7, 10, 13, 17 (= 16 + stats), 19 (= 18 + stats).
// Every variant renders the same bits.
// the tree a traversal variant walks: 0 = 2-body leaves, 1 = 4, 2 = 8
const void* trace_kernel_w16();   // trace_w16.hip
static int variant_tree(int v) { return v >= 20 ? 1 : v >= 18 ? 2 : v >= 16 ? 1 : 0; }
static const Variant& variant_table(int v) {
  static const Variant none{nullptr, false, false, 0};
  static const Variant placeholder{RT_K(SRC_LDS, SCAN_BVHQ, false), true, false, SCAN_BVHQ};   // 0: resolved per scene
  static const Variant v5{RT_K(SRC_SCALAR, SCAN_GROUP4, false), false, false, SCAN_GROUP4};
  static const Variant v12{RT_K(SRC_SCALAR, SCAN_BVH, false), false, false, SCAN_BVH};
  static const Variant v16{RT_K(SRC_LDS, SCAN_BVHQ, false), true, false, SCAN_BVHQ};
  // (8-wave workgroups: one tree image for twice the waves)
  static const Variant v18{RT_KW(SRC_LDS, SCAN_BVHO, false, 8), true, false, SCAN_BVHO, 512};
  static const Variant v22{RT_K(SRC_LDS, SCAN_BVHQ7, false), true, false, SCAN_BVHQ7, 256, 0,
                           RT_KSW(SRC_LDS, SCAN_BVHQ7, 4, 0)};
  // (22's image in 8-wave workgroups: one tree image per 8 waves, for trees
  // too big for 22's 4-wave workgroups)
  static const Variant v24{RT_KW(SRC_LDS, SCAN_BVHQ7, false, 8), true, false, SCAN_BVHQ7, 512};
  // (and in 16-wave workgroups, 64 VGPRs: 8 waves per SIMD)
  // (trace_w16.hip, compiled with its own scheduler flag)
  static const Variant v26{trace_kernel_w16(), true, false, SCAN_BVHQ7, 1024};
  // (22 on 8 x 4-pixel pools: whole pools of half the pixels for launches of
  // few 8 x 8 tiles instead of sample splits; measured slower)
  static const Variant v28{RT_KWT(SRC_LDS, SCAN_BVHQ7, false, 4, 4), true, false, SCAN_BVHQ7, 256, 4};
  switch (v) {
    case 0: return placeholder;
    case 5: return v5;
    case 12: return v12;
    case 16: return v16;
    case 18: return v18;
    case 22: return v22;
    case 24: return v24;
    case 26: return v26;
    case 28: return v28;
  }
#ifdef RTCLJ_DIAG
  if (const Variant* d = diag_variant(v)) return *d;
#endif
  return none;
}
// selectors (rt_set_variant / rt_set_schedule): atomics, read once per launch
static std::atomic<int> g_variant{0};
// tile schedule: 0 = adaptive longest-first, 1 = dispatch order
static std::atomic<int> g_schedule{0};
// BVH build: surface-area splits (default) or median splits (RTCLJ_BVH=median, for A/B)
static const bool g_bvh_sah = [] {
  const char* e = std::getenv("RTCLJ_BVH");
  return !(e && std::strcmp(e, "median") == 0);
}();
#ifdef RTCLJ_DIAG
// diagnostic build: RTCLJ_TIMELINE=1 records every launch's wave timeline
static const bool g_timeline = [] {
  const char* e = std::getenv("RTCLJ_TIMELINE");
  return e && std::atoi(e) != 0;
}();
#endif
// stats builds: per device, u64[kDbg] event counters and the u64[4 * kDbgWaves]
// wave timeline, allocated on that device at its first stats launch
constexpr int kDbg = 32;
constexpr int kDbgDevices = 64;
static std::mutex g_dbg_mu;
static unsigned long long* g_dbg[kDbgDevices] = {};
static unsigned long long* g_dbgw[kDbgDevices] = {};

}  // namespace rtclj

using namespace rtclj;

// one BVH on the device: blob = nodes | pairs | pidx (the big bodies' leaves after the tree's)
struct DTree {
  float4* blob;
  int blob_f4, off_pairs, off_pidx, big_pair0, n_big_leaves, depth, n_nodes;
  float c[3], r;
  float c0;   // kPadRmax x the tree bodies' largest radius (bvh_pad.h)
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
struct ScheduleKey {
  int width, rows, row_begin, row_tile, tile_first, tile_step, gx, gy;
};
struct Schedule {
  hipStream_t stream = nullptr;
  unsigned* cost = nullptr;
  int* order = nullptr;
  int cap = 0;          // tiles the buffers hold
  bool ready = false;   // order[] holds a permutation of key's tiles (stream-ordered)
  // The sort of the last launch's record (order_kernel, and plan_kernel for a
  // planned split) is enqueued at the start of the next launch of the shape
  // on the stream, not behind the trace kernel: a frame's launch ends with
  // its trace kernel (a one-frame process never pays the sort), and a frame
  // loop pays it once per frame as before.  sort_plan: the plan's unit count
  // (-1: no plan).
  bool sort_pending = false;
  int sort_plan = -1;
  ScheduleKey key{};
  unsigned long long* part = nullptr;   // [rows][width][3] pixel sums of split tiles (zero between launches)
  size_t part_cap = 0;                  // u64 elements
  // a split launch's trace kernel was enqueued but its finalize_kernel (which
  // re-zeroes the sums) was not: the next split launch zeroes them first
  bool part_dirty = false;
  // the stealing state (KArgs word, done, sum, owner, stealc)
  unsigned long long* word = nullptr;   // per tile
  unsigned* done = nullptr;             // per tile
  unsigned long long* sum = nullptr;    // per tile x kPoolPx x 3, zero between uses
  int steal_cap = 0;                    // tiles those hold
  int* owner = nullptr;                 // KArgs n_owner entries
  int owner_cap = 0;
  unsigned long long* stealc = nullptr; // [helpers that got samples, their first samples] since rt_steal_stats
  unsigned epoch = 0;                   // launches with sharing on this stream (mod 2^16, 1 .. 65535)
  bool epoch_started = false;
  int2* units = nullptr;                // cost-balanced split plan (plan_kernel) of the next split launch
  int units_cap = 0;
  int plan_units = -1;                  // the plan's unit count (-1: none)
  // path export (KArgs xq, xq_n): the records of a split launch's exported
  // paths, and [written, the sweep's claims] (zeroed before each launch)
  uint4* xq = nullptr;
  size_t xq_cap = 0;                    // records
  unsigned* xq_n = nullptr;
  unsigned long long xq_launches = 0;   // export launches since rt_export_stats
};
constexpr int kSchedStreams = 16;
struct ScheduleSet {
  std::mutex mu;
  int used = 0;
  Schedule s[kSchedStreams];
  static void free_entry(Schedule& e) {
    if (e.cost) (void)hipFree(e.cost);
    if (e.order) (void)hipFree(e.order);
    if (e.part) (void)hipFree(e.part);
    if (e.word) (void)hipFree(e.word);
    if (e.done) (void)hipFree(e.done);
    if (e.sum) (void)hipFree(e.sum);
    if (e.owner) (void)hipFree(e.owner);
    if (e.stealc) (void)hipFree(e.stealc);
    if (e.units) (void)hipFree(e.units);
    if (e.xq) (void)hipFree(e.xq);
    if (e.xq_n) (void)hipFree(e.xq_n);
    e = Schedule{};
  }
  void release() {
    for (int k = 0; k < used; ++k) free_entry(s[k]);
    used = 0;
  }
  // drop `stream`'s entry (its kernels have finished), keeping the others packed
  void release_stream(hipStream_t stream) {
    for (int k = 0; k < used; ++k)
      if (s[k].stream == stream) {
        free_entry(s[k]);
        if (k != used - 1) {
          s[k] = s[used - 1];
          s[used - 1] = Schedule{};
        }
        --used;
        return;
      }
  }
};

struct rt_dscene {
  int device;
  int n;
  int n_pad;
  float4* geo;
  float4* geo2;   // n_pad/2 Pairs (= n_pad float4)
  // BVHs (bvh.cpp): tree[0] 2-body leaves, tree[1] 4-body, tree[2] 8-body
  DTree tree[3];
  float4* sph;
  float4* mat;
  int* kind;
  bool unit_albedo;            // every lambertian/metal albedo channel within [-1, 1] (compact_ok)
  uint64_t uid;                // upload id (scene_uid): contexts name scenes by it, not by address
  mutable ScheduleSet sched;   // rt_launch's adaptive tile order
};
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

static int hip_fail(hipError_t e, const char* what) {
  return set_error(RT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(call)                                  \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return hip_fail(_e, #call);  \
  } while (0)

extern "C" int rt_set_variant(int v) {
  clear_error();
  if (v != 0 && !variant_table(v).fn)
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
    geo[i] = make_float4(q[0], q[1], q[2], -(r * r));
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
  // blob = nodes | pairs | pidx
  for (int k = 0; k < 3 && e == hipSuccess; ++k) {
    BvhHost& bvh = bvhs[k];
    const size_t nb = bvh.nodes.size() * sizeof(BvhNode);
    const size_t pb = bvh.pairs.size() * sizeof(float);
    // body indices: u16 for the 8-body-leaf tree (RT_MAX_SPHERES < 65535; a
    // pad's -1 -> 0xffff, never a candidate), int for the others
    const size_t isz = k == 2 ? sizeof(uint16_t) : sizeof(int);
    std::vector<uint16_t> pidx16(bvh.pidx.size());
    for (size_t i = 0; i < pidx16.size(); ++i) pidx16[i] = static_cast<uint16_t>(bvh.pidx[i]);
    const size_t ib = ((bvh.pidx.size() * isz + 15) / 16) * 16;
    std::vector<char> blob(nb + pb + ib, 0);
    if (k == 1)   // 4-body tree: inner-child refs as byte offsets (< 65536 while it fits LDS: u16 stack)
      for (BvhNode& nd : bvh.nodes)
        for (int& c : nd.child)
          if (c >= 0) c *= static_cast<int>(sizeof(BvhNode));
    std::memcpy(blob.data(), bvh.nodes.data(), nb);
    std::memcpy(blob.data() + nb, bvh.pairs.data(), pb);
    if (k == 2) std::memcpy(blob.data() + nb + pb, pidx16.data(), pidx16.size() * sizeof(uint16_t));
    else std::memcpy(blob.data() + nb + pb, bvh.pidx.data(), bvh.pidx.size() * sizeof(int));
    DTree& t = d->tree[k];
    t.blob_f4 = static_cast<int>(blob.size() / 16);
    t.off_pairs = static_cast<int>(nb);
    t.off_pidx = static_cast<int>(nb + pb);
    t.big_pair0 = bvh.big_pair0;
    t.n_big_leaves = bvh.n_big_leaves;
    t.depth = bvh.depth;
    t.n_nodes = static_cast<int>(bvh.nodes.size());
    for (int j = 0; j < 3; ++j) t.c[j] = bvh.center[j];
    t.r = bvh.radius;
    t.c0 = kPadRmax * bvh.r_max;
    e = hipMalloc(&t.blob, blob.size());
    if (e == hipSuccess) e = hipMemcpy(t.blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
  }
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
  if (d->sph) (void)hipFree(d->sph);
  if (d->mat) (void)hipFree(d->mat);
  if (d->kind) (void)hipFree(d->kind);
  delete d;
  return RT_OK;
}

// traversal stack bytes: u8 entries for the 8-body-leaf tree (tree[2], at
// most 256 nodes when its variant runs), u16 otherwise
static int stack_entries(const DTree& t, int tree) { return tree == 0 ? t.depth + 2 : std::max(t.depth, 1); }
// (threads: the workgroup's lanes, a stack row each)
static size_t stack_of(const DTree& t, int tree, int threads = 256) {
  return static_cast<size_t>(stack_entries(t, tree)) * threads * (tree == 2 ? 1 : 2);
}
static size_t lds_of(const DTree& t, int tree, int threads = 256) {
  return static_cast<size_t>(t.blob_f4) * 16 + stack_of(t, tree, threads);
}
// variant 22 (the compact image): u8 node indices, depth rows (the dead
// far-child write goes one above the top, as in 16)
static int stack_entries_compact(const DTree& t) { return std::max(t.depth, 1); }
static size_t lds_of_compact(const DTree& t, int threads) {
  return static_cast<size_t>(t.blob_f4) * 16 + static_cast<size_t>(stack_entries_compact(t)) * threads;
}
// LDS a CU can give each of 5 workgroups (160 KB / 5), less the 4-body-leaf
// kernel's static LDS (pool counter, the 64 pixels' colour sums and pixel
// table).  (Its registers allow 6; C1's 24.0 KB image fits 6 as well.)
constexpr size_t kStaticLds = 4 + kPoolPx * 3 * 8 + kPoolPx * 16 + 12;   // (the 8-body traversal: no table, 1 KB less)
constexpr size_t kLds5 = 160 * 1024 / 5 - kStaticLds;
// (variants 24 / 26's static LDS, 1.4 / 1.5 KB: the 64 pixels' u32 sums and
// keys, the wrap counts, 8 or 16 waves' compaction counters; 2 KB allowed for)
constexpr size_t kStaticLds8 = 2048;

// Tile sharing, A/B knobs read at every launch:
// RTCLJ_STEAL=0 (off: the static sample split for launches of few tiles, as
// before), RTCLJ_THIEVES (helper workgroups per workgroup slot of the
// device), RTCLJ_STEAL_MIN (unclaimed samples a tile needs for a helper to join)
static int env_int(const char* name, int dflt, int lo) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::atoi(e)) : dflt;
}
static int split_rounds() { return env_int("RTCLJ_SPLIT_ROUNDS", 3, 1); }   // (kSplitRounds above)

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

// the most splits of one tile (rt_launch's sample split, below)
constexpr int kSplitMax = 64;

// The pending sort of a stream's tile-cost record (Schedule::sort_pending):
// order_kernel, and plan_kernel for a planned split; the order is ready for
// the next launch of the shape.  Returns the launches' hipError_t.
static int sort_record(Schedule* sch, int n_tiles, int spp, hipStream_t stream) {
  unsigned* cost = sch->cost;
  int* order = sch->order;
  int n = n_tiles;
  void* sargs[] = {&cost, &order, &n};
  hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(&order_kernel), dim3(1), dim3(1024), sargs, 0, stream);
  if (e != hipSuccess) return e;
  sch->ready = true;
  sch->sort_pending = false;
  sch->plan_units = -1;
  if (sch->sort_plan > 0 && sch->units_cap >= sch->sort_plan) {
    // the next split launch's cost-balanced units, from this record
    int2* units = sch->units;
    int Uk = sch->sort_plan, smax = std::min(spp, kSplitMax);
    void* pargs[] = {&cost, &order, &n, &Uk, &smax, &units};
    e = hipLaunchKernel(reinterpret_cast<const void*>(&plan_kernel), dim3(1), dim3(1024), pargs, 0, stream);
    if (e != hipSuccess) return e;
    sch->plan_units = sch->sort_plan;
  }
  return hipSuccess;
}

// the variants of the compact image (u8 node-index stack, u32 sums)
static bool compact_variant(int v) { return v == 22 || v == 24 || v == 26 || v == 28; }

// selector -> the variant a launch on ds runs
static int resolve_variant(const rt_dscene& ds, int vsel) {
  // default: 4-body leaves, unless that tree's LDS image limits a CU below
  // 5 workgroups (160 KB / 5) and the 8-body-leaf tree's is smaller
  // (measured: 1025 bodies 12.9 vs 14.0 ms; 484: 10.8 vs 12.2); each image
  // with the stack rows of its own variant's workgroup (18: 512 lanes)
  if (vsel == 0)
    vsel = (lds_of(ds.tree[1], 1) > kLds5 && ds.tree[2].n_nodes <= 256 &&
            lds_of(ds.tree[2], 2, variant_table(18).threads) < lds_of(ds.tree[1], 1)) ? 18 : 16;
  if ((vsel == 18 || vsel == 19) && ds.tree[2].n_nodes > 256) vsel -= 2;   // u8 stack: 256 nodes at most
  // u16 stack of node LDS addresses: the kernel's static LDS (< 4 KB; 8 KB
  // allowed for) plus the node region must stay below 64 KB
  if ((vsel == 16 || vsel == 17) && ds.tree[1].n_nodes * 80 + 8192 > 65535) vsel = 12;
  // the sorted kernels: the 4-body tree's byte-offset refs in a u16 stack
  // inside a wave's exchange slots, the blob beside the exchange buffer
  if ((vsel == 20 || vsel == 21) &&
      (ds.tree[1].n_nodes * 80 > 65535 || ds.tree[1].depth + 2 > kBvhStack ||
       static_cast<size_t>(ds.tree[1].blob_f4) * 16 + kXBytes > 96 * 1024))
    vsel = 16;
  if (vsel >= 11) {
    const DTree& t = ds.tree[variant_tree(vsel)];
    if (t.depth + 2 > kBvhStack) return 5;                       // tree too deep for the stack
    // (the stack rows of the variant's own workgroup size, as launch_lds)
    if (vsel != 12 && lds_of(t, variant_tree(vsel), variant_table(vsel).threads) > 96 * 1024)
      vsel = 12;   // tree too big for LDS: 2-body leaves, global
    if (vsel == 12 && ds.tree[0].depth + 2 > kBvhStack) return 5;
  }
  if (compact_variant(vsel) && ds.tree[1].n_nodes > 256) vsel = 16;   // (u8 node indices)
  return vsel;
}

// The compact variant (22) for a launch: the 4-body tree's node indices fit
// a byte, and a pixel's u32 sum with its byte of wrap counts cannot overflow
// -- every sample's colour is at most 1 per channel (albedos within [-1, 1]:
// the sky and the dielectric give at most 1), so a channel wraps at most spp /
// 256 < 256 times for spp < 65536 (none for spp <= 255, where the kernel adds
// without counting).  Its pixel table packs no coordinates above 65535 (the
// key table plus one image row per tile row).  The default selector runs it
// wherever it applies (and an explicit 22 too); elsewhere the launch runs 16.
// Seven workgroups per CU instead of six, in 72 VGPRs without a spill.
static bool compact_ok(const rt_dscene& ds, const rt_params& p) {
  return ds.unit_albedo && ds.tree[1].n_nodes <= 256 && p.spp < 65536 && ds.tree[1].depth + 2 <= kBvhStack &&
         p.width <= 65536 && p.height <= 65536;
}
static int launch_variant(const rt_dscene& ds, const rt_params& p) {
  const int sel = g_variant.load();
  int vsel = resolve_variant(ds, sel);
  if ((sel == 0 && vsel == 16) || vsel == 22) vsel = compact_ok(ds, p) ? 22 : 16;
  // A scene the default sends to the 8-body-leaf walk (its 4-body image too
  // big for five 4-wave workgroups a CU) runs 22's compact image on the
  // 4-body walk's leaf records instead, in workgroups that share one image
  // among more waves: 16-wave workgroups (26) where two fit a CU -- 8 waves
  // per SIMD in 64 VGPRs -- else 8-wave ones (24) where three fit -- 6 per
  // SIMD, as 18.  C4: 4.295 s (26) vs 4.570 (24) vs 4.931 (18), same boxes
  // (profiles/r05/c4_v26/, c4_v24/); C2's frame on 26 instead of 22: 260.4 vs
  // 251.8 ms (a pool's 32,000 samples over 1,024 lanes drain too often).
  if (sel == 0 && vsel == 18 && compact_ok(ds, p)) {
    if (lds_of_compact(ds.tree[1], 1024) + kStaticLds8 <= 160 * 1024 / 2)
      vsel = 26;
    else if (lds_of_compact(ds.tree[1], 512) + kStaticLds8 <= 160 * 1024 / 3)
      vsel = 24;
  }
  if ((vsel == 24 || vsel == 26 || vsel == 28) && !compact_ok(ds, p)) vsel = 16;
  // RTCLJ_TH4=r (A/B knob, default 0 = never): a launch of 22 with fewer
  // 8 x 8 tiles than r x the workgroups the device holds -- a shard of a
  // multi-GPU frame -- runs 28: the same image on 8 x 4-pixel pools, whole,
  // where 22 splits every tile's samples over 2-3 workgroups.  Measured at r
  // = 2 (profiles/r06/th4/): C1's 8-rank shard 1.62 ms against 0.84 with the
  // splits, the 4-rank 1.56 against 1.37 (the whole 8 x 4 pools are 1.84
  // rounds of 3,200-sample units: the last round's long units are the tail),
  // and 28 costs 5 % more per sample on the whole C1 frame (4.95 vs 4.71 ms:
  // a pool of half the pixels drains twice as often).  DESIGN.md §6.
  if (sel == 0 && vsel == 22) {
    const int ratio = env_int("RTCLJ_TH4", 0, 0);
    if (ratio > 0) {
      const int rows = rows_out(p);
      const int64_t n8 = static_cast<int64_t>((p.width + kTile - 1) / kTile) * ((rows + kTile - 1) / kTile);
      const Variant& v22 = variant_table(22);
      const int slots = launch_slots(ds.device, v22.fn, lds_of_compact(ds.tree[1], v22.threads), v22.threads);
      if (slots > 0 && n8 < static_cast<int64_t>(ratio) * slots) vsel = 28;
    }
  }
  return vsel;
}

extern "C" int rt_resolve_variant(const rt_dscene* ds) { return ds ? resolve_variant(*ds, g_variant.load()) : -1; }

// dynamic LDS of a launch of variant vsel on ds
static size_t launch_lds(const rt_dscene& ds, int vsel) {
  const Variant& v = variant_table(vsel);
  if (v.scan == SCAN_BVHS) return static_cast<size_t>(ds.tree[1].blob_f4) * 16 + kXBytes;   // blob | exchange
  if (compact_variant(vsel)) return lds_of_compact(ds.tree[1], v.threads);
  if (vsel >= 11) {
    const DTree& tr = ds.tree[variant_tree(vsel)];
    return v.lds ? lds_of(tr, variant_tree(vsel), v.threads) : stack_of(tr, variant_tree(vsel), v.threads);
  }
  return v.lds ? static_cast<size_t>(ds.n_pad) * sizeof(float4) : 0;
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
  const void* fn = variant_table(vsel).fn;
  if (!fn) return set_error(RT_E_ARG, "rt_launch_occupancy: no kernel for variant " + std::to_string(vsel));
  const size_t lds = launch_lds(*ds, vsel);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  int blocks = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, variant_table(vsel).threads, lds));
  hipFuncAttributes fa{};
  HIP_TRY(hipFuncGetAttributes(&fa, fn));
  out4[0] = blocks * variant_table(vsel).threads / 256;   // (in 256-thread workgroups) per CU
  out4[1] = fa.numRegs;           // VGPRs per lane
  out4[2] = static_cast<int>(lds + fa.sharedSizeBytes);   // LDS bytes per workgroup
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

// Sample split (rt_launch): split every tile of a launch with fewer tiles
// than kSplitRounds (RTCLJ_SPLIT_ROUNDS, default 3) x (resident workgroups), into enough splits to reach that
// (at most kSplitMax).  tools/shard_time.py on C1's 1/2/4/8-GPU shards
// (profiles/r02/shard_split_rounds.txt): 3-4 rounds best (8 GPUs: 5.88x at 3,
// 5.72x at 4, 5.30x at 6, 3.96x at 16; unsplit 2.57x)
// (kSplitMax, the most splits of a tile: defined above sort_record)

namespace rtclj {
int fill_async(void* p, int byte_value, size_t bytes, void* stream) {
  if (bytes == 0) return hipSuccess;
  if (bytes % 4 != 0) return hipErrorInvalidValue;   // (every buffer the product fills is whole words)
  uint32_t* w = static_cast<uint32_t*>(p);
  uint32_t v = static_cast<uint32_t>(byte_value & 0xff) * 0x01010101u;
  size_t n = bytes / 4;
  const size_t blocks = std::min<size_t>((n + 255) / 256, 2048);
  void* args[] = {&w, &v, &n};
  return hipLaunchKernel(reinterpret_cast<const void*>(&fill_kernel), dim3(static_cast<unsigned>(blocks)), dim3(256),
                         args, 0, static_cast<hipStream_t>(stream));
}

int quantize_launch(const float* d_lin, uint8_t* d_out, size_t n, void* stream) {
  static const QThr thr = [] {
    QThr t;
    std::memcpy(t.t, quantize_thresholds(), sizeof t.t);
    return t;
  }();
  if (n == 0) return hipSuccess;
  const size_t blocks = std::min<size_t>((n + 255) / 256, 4096);
  QThr q = thr;
  const float* in = d_lin;
  uint8_t* out = d_out;
  void* args[] = {&in, &out, &n, &q};
  return hipLaunchKernel(reinterpret_cast<const void*>(&quantize_kernel), dim3(static_cast<unsigned>(blocks)),
                         dim3(256), args, 0, static_cast<hipStream_t>(stream));
}
}  // namespace rtclj

// rt_launch, and rt_launch_accum's pass (acc_sums: the accumulator's
// [rows][width][3] sums; d_out NULL).  A pass is the launch with no whole
// tiles (n_whole = 0: every unit, one per tile or `split` per tile, adds its
// integer sums to part[] = acc_sums by atomics) and no finalize_kernel behind
// it; the stream's own part buffer and its part_dirty flag are left alone.
// rt_adapt_step's pass adds `active`, a device list of n_active tiles: the
// launch's tile order, whose length stands for the tile count in the split and
// the unit count -- the same launch with a shorter order.  It needs 8 x 8
// tiles, and neither reads nor writes the stream's record (no cost, no order).
static int launch_impl(const rt_dscene* ds, const rt_camera* c, const rt_params* p, float* d_out,
                       uint64_t* d_counters, void* hip_stream, unsigned long long* acc_sums,
                       const char* who = "rt_launch", const int* active = nullptr, int n_active = 0) {
  if (!ds || !c || !p || (!d_out && !acc_sums)) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  if (p->width <= 0 || p->height <= 0 || p->spp < 0 || p->spp > RT_MAX_SPP ||
      (p->flags & ~(RT_FLAG_REALM | RT_FLAG_STREAMED | RT_FLAG_REJECTION_SAMPLERS)) != 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad width/height/spp/flags");
  const int rows = rows_out(*p);
  if (rows < 0) return set_error(RT_E_ARG, std::string(who) + ": bad row selection");
  KArgs a{};
  a.geo = ds->geo;
  a.geo2 = reinterpret_cast<const Pair*>(ds->geo2);
  a.sph = ds->sph;
  a.mat = ds->mat;
  a.kind = ds->kind;
  a.out = d_out;
  a.counters = reinterpret_cast<unsigned long long*>(d_counters);
  std::memcpy(a.cam + 0, c->center, 12);
  std::memcpy(a.cam + 3, c->p00, 12);
  std::memcpy(a.cam + 6, c->du, 12);
  std::memcpy(a.cam + 9, c->dv, 12);
  std::memcpy(a.cam + 12, c->disk_u, 12);
  std::memcpy(a.cam + 15, c->disk_v, 12);
  a.defocus = c->defocus ? 1 : 0;
  a.n = ds->n;
  a.n_pad = ds->n_pad;
  a.width = p->width;
  a.rows_out = rows;
  a.row_begin = p->row_begin;
  a.row_tile = p->row_tile > 0 ? p->row_tile : 8;
  a.tile_first = p->tile_first;
  a.tile_step = p->tile_step;
  a.spp = p->spp;
  a.sample_begin = p->sample_begin;
  a.max_depth = p->max_depth;
  a.realm = (p->flags & RT_FLAG_REALM) ? 1 : 0;
  // the loop-free samplers unless the caller asks for the reference's rejection loops
  a.sampler = (p->flags & RT_FLAG_REJECTION_SAMPLERS) ? 0 : (RT_SAMPLER_SPHERE | RT_SAMPLER_DISK);
  a.key = seed_key(p->seed);
  if (rows == 0) return RT_OK;
  HIP_TRY(hipSetDevice(ds->device));
  int vsel = launch_variant(*ds, *p);
  if (variant_table(vsel).scan == SCAN_BVHS && p->max_depth > 1023) vsel = 16;   // (a path's depth left: 10 bits in the exchange)
  const Variant& v = variant_table(vsel);
  if (!v.fn) return set_error(RT_E_ARG, std::string(who) + ": no kernel for variant " + std::to_string(vsel));
  const DTree& tr = ds->tree[variant_tree(vsel)];
  a.bvh_blob = tr.blob;
  a.bvh_blob_f4 = tr.blob_f4;
  a.bvh_off_pairs = tr.off_pairs;
  a.bvh_off_pidx = tr.off_pidx;
  a.big_pair0 = tr.big_pair0;
  a.n_big_leaves = tr.n_big_leaves;
  // entries per lane: the ordered traversal (trees 1, 2) holds at most depth
  // (a node on level L has L - 1 ancestors; the dead far-child write goes one
  // above them); tree 0 also serves the while-while variants (depth + 2)
  a.bvh_stack = compact_variant(vsel) ? stack_entries_compact(tr) : stack_entries(tr, variant_tree(vsel));
  for (int k = 0; k < 3; ++k) a.bvh_c[k] = tr.c[k];
  a.bvh_r = tr.r;
  a.bvh_c0 = tr.c0;
  // drain compaction: a post holds as many paths as a wave's stack slice has
  // room for (RTCLJ_COMPACT: post at or below that many paths; 0 off)
  {
    const int words = a.bvh_stack * 16 * (v.scan == SCAN_BVHO || v.scan == SCAN_BVHQ7 ? 1 : 2);   // a wave's stack slice
    a.mb_paths = std::min(32, words / kMbFields);
    a.compact = is_bvh_scan(v.scan) ? std::min(a.mb_paths, env_int("RTCLJ_COMPACT", a.mb_paths, 0)) : 0;
  }
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int th = variant_rows(v);   // the variant's tile rows
  const int gx = (p->width + kTile - 1) / kTile, gy = (rows + th - 1) / th;
  const dim3 block(v.threads);
  if (active && (th != kTile || n_active <= 0 || n_active > gx * gy))
    return set_error(RT_E_ARG, std::string(who) + ": variant " + std::to_string(vsel) + " has no 8 x 8 tiles");
  const int n_tiles = active ? n_active : gx * gy;
  a.tiles_x = gx;
  if (v.stats) {
    const int rc = dbg_buffers(ds->device, &a.dbg, &a.dbgw);
    if (rc != RT_OK) return rc;
  }
#ifdef RTCLJ_DIAG
  else if (g_timeline) {   // wave timeline only (rt_debug_waves), no counters
    unsigned long long* unused = nullptr;
    const int rc = dbg_buffers(ds->device, &unused, &a.dbgw);
    if (rc != RT_OK) return rc;
  }
#endif
#ifdef RTCLJ_DIAG
  // (diagnostic: RTCLJ_LDS_PAD bytes of dynamic LDS added to the launch, to
  // measure the kernel at fewer workgroups per CU)
  const size_t lds = launch_lds(*ds, vsel) + static_cast<size_t>(env_int("RTCLJ_LDS_PAD", 0, 0));
#else
  const size_t lds = launch_lds(*ds, vsel);
#endif
  if (lds > 64 * 1024) {
    HIP_TRY(hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    if (v.sweep) HIP_TRY(hipFuncSetAttribute(v.sweep, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  }
  // the stream's entry: adaptive schedule and split partial sums
  Schedule* sch = nullptr;
  std::unique_lock<std::mutex> sched_lock;
  if (!active) {
    ScheduleSet& set = ds->sched;
    sched_lock = std::unique_lock<std::mutex>(set.mu);
    for (int k = 0; k < set.used && !sch; ++k)
      if (set.s[k].stream == stream) sch = &set.s[k];
    if (!sch && set.used < kSchedStreams) {
      sch = &set.s[set.used++];
      sch->stream = stream;
    }
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
  int split = 1, n_whole = n_tiles;
  const bool steal = sch && env_int("RTCLJ_STEAL", 1, 0) != 0 && !v.stats && v.scan != SCAN_BVHS;
  if ((sch || acc_sums) && p->spp > 1) {
    if (const char* e = std::getenv("RTCLJ_SPLIT")) {
      split = std::max(1, std::atoi(e));
    } else {
      const int slots = launch_slots(ds->device, v.fn, lds, v.threads);
      // (28: its pools are the split's answer already; they split only when
      // fewer than RTCLJ_TH4_SPLIT_ROUNDS (1) rounds of them fill the device)
      const int rounds = vsel == 28 ? env_int("RTCLJ_TH4_SPLIT_ROUNDS", 1, 1) : split_rounds();
      const int64_t want = static_cast<int64_t>(rounds) * slots;
      if (slots > 0 && n_tiles < want) {
        split = static_cast<int>((want + n_tiles - 1) / n_tiles);
        // frames in flight: the next frame fills this launch's tail, so two
        // rounds of workgroups suffice (at least 2 splits: an unsplit heavy
        // tile would outlive two frames).  C1's 8-GPU shard, 2 streams:
        // 0.817 ms per frame at split 2 vs 0.87 at 3 (profiles/r03/shard_matrix_*.txt)
        if (p->flags & RT_FLAG_STREAMED)
          split = std::max(2, static_cast<int>((2 * static_cast<int64_t>(slots) + n_tiles - 1) / n_tiles));
      }
    }
    split = std::min(split, std::min(p->spp, kSplitMax));
    if (split > 1) n_whole = 0;
  }
  if (acc_sums) n_whole = 0;   // an accumulating pass: every unit's sums go to part[]
  a.split = split;
  a.n_whole = n_whole;
  a.rt_magic = magic64(a.row_tile);
  const int64_t n_units64 = n_whole + static_cast<int64_t>(n_tiles - n_whole) * split;
  if (n_units64 > INT_MAX) return set_error(RT_E_ARG, std::string(who) + ": frame too large");
  const int n_units = static_cast<int>(n_units64);
  const size_t n_elems = static_cast<size_t>(rows) * p->width * 3;
  if (acc_sums) {
    a.part = acc_sums;
  } else if (split > 1) {
    // the split tiles' integer sums: one u64 per channel, added to by the
    // splits, converted and zeroed by finalize_kernel
    const size_t need = n_elems;
    if (sch->part_cap < need) {   // grow: this stream's kernels may still read the old buffer
      HIP_TRY(hipStreamSynchronize(stream));
      if (sch->part) (void)hipFree(sch->part);
      sch->part = nullptr;
      sch->part_cap = 0;
      HIP_TRY(hipMalloc(&sch->part, need * sizeof(unsigned long long)));
      HIP_TRY(static_cast<hipError_t>(fill_async(sch->part, 0, need * sizeof(unsigned long long), stream)));
      sch->part_cap = need;
      sch->part_dirty = false;
    }
    if (sch->part_dirty) {   // an earlier launch failed between its trace and finalize kernels
      HIP_TRY(static_cast<hipError_t>(fill_async(sch->part, 0, sch->part_cap * sizeof(unsigned long long), stream)));
      sch->part_dirty = false;
    }
    a.part = sch->part;
  }
  // adaptive schedule: dispatch tiles longest first, by the durations the
  // previous launches of this launch shape on this scene and stream measured
  // (each launch's added to half the record before it)
  bool new_shape = false;
  if (sch) {
    ScheduleKey key{};
    key.width = a.width;
    key.rows = a.rows_out;
    key.row_begin = a.row_begin;
    key.row_tile = a.row_tile;
    key.tile_first = a.tile_first;
    key.tile_step = a.tile_step;
    key.gx = gx;
    key.gy = gy;
    if (std::memcmp(&sch->key, &key, sizeof key) != 0) {
      sch->ready = false;
      sch->sort_pending = false;   // (that record was another shape's)
      sch->key = key;
      new_shape = true;
    }
  }
  // the fills this launch needs before its trace kernel, as one launch
  FillSet fills;
  bool first_order = false;   // a shape's first launch in a heuristic order
  if (sch && g_schedule.load() == 0) {
    if (sch->cap < n_tiles) {   // grow: this stream's kernels may still read the old buffers
      HIP_TRY(hipStreamSynchronize(stream));
      if (sch->cost) (void)hipFree(sch->cost);
      if (sch->order) (void)hipFree(sch->order);
      sch->cost = nullptr;
      sch->order = nullptr;
      sch->cap = 0;
      sch->ready = false;
      sch->sort_pending = false;
      HIP_TRY(hipMalloc(&sch->cost, n_tiles * sizeof(unsigned)));
      HIP_TRY(hipMalloc(&sch->order, n_tiles * sizeof(int)));
      sch->cap = n_tiles;
    }
    // the previous launch's record, sorted now (stream-ordered after it)
    if (sch->sort_pending) HIP_TRY(static_cast<hipError_t>(sort_record(sch, n_tiles, p->spp, stream)));
    if (sch->ready) {
      a.tile_order = sch->order;
    } else if (env_int("RTCLJ_FIRST_ORDER", 1, 0) == 1) {
      // No record yet: the tiles bottom-up.  The reference's scenes (and
      // C1-C4) put the ground and its bodies below the sky: the expensive
      // tiles start first and the launch ends on sky tiles, where row-major
      // order ended on the ground's.  C1's first frame of a shape 5.13-5.19
      // ms against 5.25 row-major (tools/first_frame.py, 9 pairs, two
      // rounds; profiles/r06/first_order/); RTCLJ_FIRST_ORDER=0: row-major.
      // Tile sharing still balances the tail, as in plain order.
      int* order = sch->order;
      int n = n_tiles;
      void* oargs[] = {&order, &n};
      HIP_TRY(hipLaunchKernel(reinterpret_cast<const void*>(&iota_rev_kernel), dim3(static_cast<unsigned>((n + 255) / 256)),
                              dim3(256), oargs, 0, stream));
      a.tile_order = sch->order;
      first_order = true;
    }
    a.tile_cost = sch->cost;
    // a split launch in the recorded order: with RTCLJ_SPLIT_PLAN=1, the
    // cost-balanced units the previous launch of the shape planned (when it
    // planned this many).  Off by default: C1's 8-GPU shard 1.10-1.15 ms
    // against 0.99-1.02 with uniform splits, the 4-GPU one 1.93 vs 1.69
    // (profiles/r04/split_plan/; round 2's cost-sized splits lost the same
    // way): a heavy tile's many short pools each end with idle lanes.
    if (split > 1 && sch->ready && sch->plan_units == n_units - n_whole && env_int("RTCLJ_SPLIT_PLAN", 0, 0) != 0)
      a.unit_tab = sch->units;
    // the costs decay (order_kernel halves them after sorting): zeroed only
    // when this launch shape starts a new history
    if (!sch->ready) fills.add(sch->cost, 0, n_tiles * sizeof(unsigned));
  }
  if (active) a.tile_order = active;
  // the grid: the units, then (stealing) the thieves, dispatched last, i.e.
  // as the units' slots free up in the launch's tail
  int64_t grid = n_units;
  // Sharing balances a launch whose tiles have no cost record (plain order:
  // a process's or a shape's first frame).  In the recorded longest-first
  // order the cheap tiles come last and the tail is short without it (C1
  // 5.94 ms either way), while its claims and helpers' scans are HBM atomics
  // (C1: 31 vs 11 MB per launch; profiles/r04/share_rounds/): off there
  // unless RTCLJ_SHARE_RECORDED=1.
  if (steal && split == 1 && !acc_sums && (!a.tile_order || first_order || env_int("RTCLJ_SHARE_RECORDED", 0, 0) != 0)) {
    const int slots = std::max(1, launch_slots(ds->device, v.fn, lds, v.threads));
    const int n_owner = 2 * slots;   // owner entries: twice the resident workgroups
    // (at most 32 per slot: a tile's helper count stays below 2^16)
    grid += static_cast<int64_t>(std::min(32, env_int("RTCLJ_THIEVES", 4, 0))) * slots;
    if (grid > INT_MAX) grid = n_units;
    if (!sch->stealc) {
      HIP_TRY(hipMalloc(&sch->stealc, 2 * sizeof(unsigned long long)));
      HIP_TRY(static_cast<hipError_t>(fill_async(sch->stealc, 0, 2 * sizeof(unsigned long long), stream)));
    }
    if (sch->steal_cap < n_tiles) {   // grow: this stream's kernels may still use the old buffers
      HIP_TRY(hipStreamSynchronize(stream));
      if (sch->word) (void)hipFree(sch->word);
      if (sch->done) (void)hipFree(sch->done);
      if (sch->sum) (void)hipFree(sch->sum);
      sch->word = nullptr;
      sch->done = nullptr;
      sch->sum = nullptr;
      sch->steal_cap = 0;
      const size_t nsum = static_cast<size_t>(n_tiles) * kPoolPx * 3;
      HIP_TRY(hipMalloc(&sch->word, n_tiles * sizeof(unsigned long long)));
      HIP_TRY(hipMalloc(&sch->done, n_tiles * sizeof(unsigned)));
      HIP_TRY(hipMalloc(&sch->sum, nsum * sizeof(unsigned long long)));
      // words 0: lo = hi, nothing to steal until an owner publishes; sums
      // and done counts 0 (the kernel keeps them so between uses)
      HIP_TRY(static_cast<hipError_t>(fill_async(sch->word, 0, n_tiles * sizeof(unsigned long long), stream)));
      HIP_TRY(static_cast<hipError_t>(fill_async(sch->done, 0, n_tiles * sizeof(unsigned), stream)));
      HIP_TRY(static_cast<hipError_t>(fill_async(sch->sum, 0, nsum * sizeof(unsigned long long), stream)));
      sch->steal_cap = n_tiles;
      new_shape = true;
    }
    if (sch->owner_cap != n_owner) {
      HIP_TRY(hipStreamSynchronize(stream));
      if (sch->owner) (void)hipFree(sch->owner);
      sch->owner = nullptr;
      sch->owner_cap = 0;
      HIP_TRY(hipMalloc(&sch->owner, n_owner * sizeof(int)));
      sch->owner_cap = n_owner;
      new_shape = true;
    }
    if (!sch->epoch_started) {   // (RTCLJ_EPOCH_START: tests start a stream near the wrap)
      sch->epoch = static_cast<unsigned>(std::min(0xffff, env_int("RTCLJ_EPOCH_START", 1, 1)) - 1);
      sch->epoch_started = true;
    }
    sch->epoch = (sch->epoch + 1) & 0xffffu;
    if (sch->epoch == 0) {   // wrapped: no word or owner entry may carry the epoch's last use
      sch->epoch = 1;
      new_shape = true;
    }
    a.epoch = sch->epoch;
    // a new shape (or a wrap): no tile is being run, and no word holds this
    // launch's epoch.  (Old owner entries would only name words of other
    // epochs, but tile indices of another shape may exceed this one's; a word
    // last published 65,535 launches ago carries the epoch a wrap reuses.)
    if (new_shape) {
      fills.add(sch->owner, 0xff, n_owner * sizeof(int));
      fills.add(sch->word, 0, n_tiles * sizeof(unsigned long long));
    }
    // owners publish only in the launch's last RTCLJ_SHARE_ROUNDS rounds of
    // units (default 2; a round = the workgroups the device holds at once.
    // C4 plain order: WRITE_SIZE 2.90 GB per launch at every round, 0.44 at
    // 2, 0.60 at 3; C1's timing the same at 1, 2, 3 or every round:
    // profiles/r04/share_rounds/)
    a.share_from = static_cast<int>(std::max<int64_t>(
        0, n_units - static_cast<int64_t>(env_int("RTCLJ_SHARE_ROUNDS", 2, 0)) * slots));
    a.word = sch->word;
    a.done = sch->done;
    a.sum = sch->sum;
    a.owner = sch->owner;
    a.n_owner = n_owner;
    a.stealc = sch->stealc;
    a.steal_min = env_int("RTCLJ_STEAL_MIN", 256, 1);
    // claims of up to 1024 samples in the record's longest-first order (the
    // heavy tiles start first: fewer claims, 6.03 -> 6.00 ms on C1); in plain
    // order up to 1/48 of the tile's pool (0: the kernel's per-pool rule; C1's
    // 6,400: 128 -- helpers then need small claims to balance the tail;
    // C4's 64,000: 1024)
    a.batch_max = env_int("RTCLJ_BATCH_MAX", (a.tile_order && !first_order) ? 1024 : 0, 0);
  }
  a.n_units = n_units;
  // a wave's claims on an unshared pool: guided (an eighth of what is left
  // past its last batch), 64 .. RTCLJ_LDS_BATCH (default 256; fixed 64-index
  // batches were round 3's: C1 5.960 -> 5.916 ms, C2 287.9 -> 286.1 ms,
  // profiles/r04/lds_batch/)
  a.lds_batch_max = std::max(64, env_int("RTCLJ_LDS_BATCH", 256, 64));
  // Path export for split launches (KArgs xq; RTCLJ_EXPORT=1, A/B): a wave
  // whose batches are spent and which holds at most RTCLJ_EXPORT_LIM paths
  // (default 64: as soon as its batches are spent) writes them out and
  // leaves, so a unit's workgroup frees its slot without draining; the sweep
  // launch runs the records.  At most one record per thread of a unit.
  const bool xport = sch && split > 1 && v.sweep && env_int("RTCLJ_EXPORT", 0, 0) != 0;
  if (xport) {
    const size_t need = static_cast<size_t>(n_units) * v.threads;
    if (sch->xq_cap < need) {   // grow: this stream's kernels may still read the old records
      HIP_TRY(hipStreamSynchronize(stream));
      if (sch->xq) (void)hipFree(sch->xq);
      sch->xq = nullptr;
      sch->xq_cap = 0;
      HIP_TRY(hipMalloc(&sch->xq, need * 4 * sizeof(uint4)));
      sch->xq_cap = need;
    }
    if (!sch->xq_n) HIP_TRY(hipMalloc(&sch->xq_n, 2 * sizeof(unsigned)));
    fills.add(sch->xq_n, 0, 2 * sizeof(unsigned));
    a.xq = sch->xq;
    a.xq_n = sch->xq_n;
    a.compact = std::min(64, env_int("RTCLJ_EXPORT_LIM", 64, 1));
    ++sch->xq_launches;
  }
  if (fills.count) {
    size_t most = 0;
    for (int k = 0; k < fills.count; ++k) most = std::max(most, fills.n[k]);
    const size_t blocks = std::max<size_t>(1, std::min<size_t>((most + 255) / 256, 2048));
    void* fa[] = {&fills};
    HIP_TRY(hipLaunchKernel(reinterpret_cast<const void*>(&fill_set_kernel), dim3(static_cast<unsigned>(blocks)),
                            dim3(256), fa, 0, stream));
  }
  void* args[] = {&a};
  if (split > 1 && !acc_sums) sch->part_dirty = true;   // (cleared once finalize_kernel is enqueued)
  HIP_TRY(hipLaunchKernel(v.fn, dim3(static_cast<unsigned>(grid)), block, args, lds, stream));
  if (xport) {
    // the sweep: one workgroup per slot the device holds, each starting on
    // its own 256 records and claiming more; a workgroup past the records
    // leaves at once.  It adds into part[], so it runs before finalize_kernel.
    KArgs b = a;
    b.word = nullptr;
    b.tile_cost = nullptr;
    b.tile_order = nullptr;
    b.unit_tab = nullptr;
    b.compact = is_bvh_scan(v.scan) ? std::min(b.mb_paths, env_int("RTCLJ_COMPACT", b.mb_paths, 0)) : 0;
    const int sw = std::max(1, launch_slots(ds->device, v.sweep, lds, v.threads));
    void* bargs[] = {&b};
    HIP_TRY(hipLaunchKernel(v.sweep, dim3(static_cast<unsigned>(sw)), block, bargs, lds, stream));
  }
  if (split > 1 && !acc_sums) {
    unsigned long long* part = a.part;
    const int* order = a.tile_order;
    int nw = n_whole, tx = gx, tht = th, w = p->width, nr = rows, spp = p->spp, realm = a.realm;
    float* out = d_out;
    void* fargs[] = {&part, &order, &nw, &tx, &tht, &w, &nr, &out, &spp, &realm};
    HIP_TRY(hipLaunchKernel(reinterpret_cast<const void*>(&finalize_kernel), dim3(n_tiles - n_whole), dim3(kTile * 3 * th),
                            fargs, 0, stream));
    sch->part_dirty = false;
  }
  if (a.tile_cost) {
    // this record's sort, at the next launch of the shape on the stream
    // (RTCLJ_SORT_EAGER=1, A/B: right behind this launch, as before round 6;
    // within noise on every bench.py leg, profiles/r06/sort_ab/)
    sch->sort_pending = true;
    sch->ready = false;
    sch->sort_plan = -1;
    if (split > 1 && n_whole == 0 && env_int("RTCLJ_SPLIT_PLAN", 0, 0) != 0) {
      const int U = n_units;
      if (sch->units_cap < U) {   // grow: this stream's kernels may still read the old plan
        HIP_TRY(hipStreamSynchronize(stream));
        if (sch->units) (void)hipFree(sch->units);
        sch->units = nullptr;
        sch->units_cap = 0;
        HIP_TRY(hipMalloc(&sch->units, U * sizeof(int2)));
        sch->units_cap = U;
      }
      sch->sort_plan = U;
    }
    if (env_int("RTCLJ_SORT_EAGER", 0, 0) != 0) HIP_TRY(static_cast<hipError_t>(sort_record(sch, n_tiles, p->spp, stream)));
  }
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

extern "C" int rt_launch(const rt_dscene* ds, const rt_camera* c, const rt_params* p, float* d_out,
                         uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!d_out) return set_error(RT_E_ARG, "rt_launch: NULL argument");
  return launch_impl(ds, c, p, d_out, d_counters, hip_stream, nullptr);
}

// ---- progressive rendering: the accumulator (rt.h) ------------------------
// The frame's integer sums outlive the launches: rows x width x 3 u64 on the
// scene's device, and the samples per pixel they hold (host side; a pass
// counts when it is enqueued).  mu orders the count's updates and the one
// staging buffer of rt_accum_add.
struct rt_accum {
  int device = 0;
  rt_params shape{};   // width, height and the row selection (row_tile resolved)
  size_t n = 0;        // sums: rows_out x width x 3
  unsigned long long* sums = nullptr;
  unsigned long long* stage = nullptr;   // rt_accum_add's copy of the caller's sums (n, on first use)
  mutable std::mutex mu;
  int64_t samples = 0;
};
constexpr int64_t kAccumMaxSamples = 0xffffffffll;   // the sample index is a uint32

static rt_params accum_shape(const rt_params& p) {
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
static bool same_shape(const rt_params& a, const rt_params& b) {
  return a.width == b.width && a.height == b.height && a.row_begin == b.row_begin && a.row_end == b.row_end &&
         a.row_tile == b.row_tile && a.tile_first == b.tile_first && a.tile_step == b.tile_step;
}

extern "C" int rt_accum_create(const rt_dscene* ds, const rt_params* shape, rt_accum** out) {
  clear_error();
  if (!ds || !shape || !out) return set_error(RT_E_ARG, "rt_accum_create: NULL argument");
  *out = nullptr;
  const int rows = rows_out(*shape);
  if (shape->width <= 0 || shape->height <= 0 || rows <= 0)
    return set_error(RT_E_ARG, "rt_accum_create: bad width/height/row selection");
  HIP_TRY(hipSetDevice(ds->device));
  rt_accum* acc = new rt_accum;
  acc->device = ds->device;
  acc->shape = accum_shape(*shape);
  acc->n = static_cast<size_t>(rows) * shape->width * 3;
  // zeroed before the call returns: the first pass may come on any stream
  hipError_t e = hipMalloc(&acc->sums, acc->n * sizeof(unsigned long long));
  if (e == hipSuccess) e = static_cast<hipError_t>(fill_async(acc->sums, 0, acc->n * sizeof(unsigned long long), nullptr));
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    if (acc->sums) (void)hipFree(acc->sums);
    delete acc;
    return hip_fail(e, "rt_accum_create");
  }
  *out = acc;
  return RT_OK;
}

extern "C" int rt_accum_free(rt_accum* acc) {
  if (!acc) return RT_OK;
  (void)hipSetDevice(acc->device);
  if (acc->sums) (void)hipFree(acc->sums);
  if (acc->stage) (void)hipFree(acc->stage);
  delete acc;
  return RT_OK;
}

extern "C" int rt_accum_clear(rt_accum* acc, void* hip_stream) {
  clear_error();
  if (!acc) return set_error(RT_E_ARG, "rt_accum_clear: NULL argument");
  std::lock_guard<std::mutex> lk(acc->mu);
  HIP_TRY(hipSetDevice(acc->device));
  HIP_TRY(static_cast<hipError_t>(fill_async(acc->sums, 0, acc->n * sizeof(unsigned long long), hip_stream)));
  acc->samples = 0;
  return RT_OK;
}

extern "C" int64_t rt_accum_samples(const rt_accum* acc) {
  if (!acc) return 0;
  std::lock_guard<std::mutex> lk(acc->mu);
  return acc->samples;
}

extern "C" int rt_launch_accum(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_accum* acc,
                               uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!ds || !c || !p || !acc) return set_error(RT_E_ARG, "rt_launch_accum: NULL argument");
  if (ds->device != acc->device)
    return set_error(RT_E_ARG, "rt_launch_accum: the scene is on device " + std::to_string(ds->device) +
                                   ", the accumulator on device " + std::to_string(acc->device));
  if (!same_shape(accum_shape(*p), acc->shape))
    return set_error(RT_E_ARG, "rt_launch_accum: width/height/row selection differ from the accumulator's");
  std::lock_guard<std::mutex> lk(acc->mu);
  if (p->spp > 0 && acc->samples + p->spp > kAccumMaxSamples)
    return set_error(RT_E_ARG, "rt_launch_accum: more than 2^32 - 1 samples per pixel");
  const int rc = launch_impl(ds, c, p, nullptr, d_counters, hip_stream, acc->sums, "rt_launch_accum");
  if (rc == RT_OK) acc->samples += p->spp;
  return rc;
}

static int accum_resolve(const rt_accum* acc, int flags, float* d_f, uint8_t* d_u8, void* hip_stream,
                         const char* who) {
  clear_error();
  if (!acc || (!d_f && !d_u8)) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  if ((flags & ~(RT_FLAG_REALM | RT_FLAG_STREAMED | RT_FLAG_REJECTION_SAMPLERS)) != 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad flags");
  static const QThr thr = [] {
    QThr t;
    std::memcpy(t.t, quantize_thresholds(), sizeof t.t);
    return t;
  }();
  int64_t count;
  {
    std::lock_guard<std::mutex> lk(acc->mu);
    count = acc->samples;
  }
  HIP_TRY(hipSetDevice(acc->device));
  const unsigned long long* sums = acc->sums;
  size_t n = acc->n;
  float nf = static_cast<float>(count > 0 ? count : 1);   // RN(float(n))
  int realm = (flags & RT_FLAG_REALM) ? 1 : 0;
  QThr q = thr;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((n / 2 + 255) / 256, 4096));
  void* args[] = {&sums, &n, &nf, &realm, &d_f, &d_u8, &q};
  HIP_TRY(hipLaunchKernel(reinterpret_cast<const void*>(&resolve_kernel), dim3(static_cast<unsigned>(blocks)), dim3(256),
                          args, 0, static_cast<hipStream_t>(hip_stream)));
  return RT_OK;
}

extern "C" int rt_accum_resolve(const rt_accum* acc, int flags, float* d_out, void* hip_stream) {
  return accum_resolve(acc, flags, d_out, nullptr, hip_stream, "rt_accum_resolve");
}

extern "C" int rt_accum_resolve_u8(const rt_accum* acc, int flags, uint8_t* d_out, void* hip_stream) {
  return accum_resolve(acc, flags, nullptr, d_out, hip_stream, "rt_accum_resolve_u8");
}

extern "C" int rt_accum_read(const rt_accum* acc, uint64_t* host_sums, void* hip_stream) {
  clear_error();
  if (!acc || !host_sums) return set_error(RT_E_ARG, "rt_accum_read: NULL argument");
  HIP_TRY(hipSetDevice(acc->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_sums, acc->sums, acc->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_accum_add(rt_accum* acc, const uint64_t* host_sums, int64_t samples, void* hip_stream) {
  clear_error();
  if (!acc || !host_sums) return set_error(RT_E_ARG, "rt_accum_add: NULL argument");
  std::lock_guard<std::mutex> lk(acc->mu);
  if (samples < 0 || samples > kAccumMaxSamples || acc->samples + samples > kAccumMaxSamples)
    return set_error(RT_E_ARG, "rt_accum_add: samples negative, or more than 2^32 - 1 per pixel in all");
  HIP_TRY(hipSetDevice(acc->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (!acc->stage) HIP_TRY(hipMalloc(&acc->stage, acc->n * sizeof(unsigned long long)));
  HIP_TRY(hipMemcpyAsync(acc->stage, host_sums, acc->n * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  unsigned long long* sums = acc->sums;
  const unsigned long long* add = acc->stage;
  size_t n = acc->n;
  const size_t blocks = std::min<size_t>((n + 255) / 256, 4096);
  void* args[] = {&sums, &add, &n};
  HIP_TRY(hipLaunchKernel(reinterpret_cast<const void*>(&accum_add_kernel), dim3(static_cast<unsigned>(blocks)), dim3(256),
                          args, 0, stream));
  // the caller's array and the staging copy are free again when this returns
  HIP_TRY(hipStreamSynchronize(stream));
  acc->samples += samples;
  return RT_OK;
}

// ---- adaptive sampling: two half accumulators and a stopping rule (rt.h) -----
// h[0], h[1]: the sums of the even and the odd steps, in the accumulator's
// layout; counts: samples per pixel of each 8 x 8 tile of the output rows;
// list[cur]: the tiles still traced, n_active of them holding px_active
// pixels.  An evaluation (adapt_eval_kernel behind an odd step) writes
// list[cur ^ 1] and counts its length and pixels in state[2 * (gen & 1) ..];
// that pair is copied to `pinned` behind it, and the next step waits for `ev`
// and takes the two numbers from there: the grid of its launch depends on
// them.  The pairs alternate so that a kernel zeroes the one the evaluation
// after it counts in.  mu orders the entries' host state.
struct rt_adapt {
  int device = 0;
  rt_params shape{};
  rt_adapt_opts opts{};
  int rows = 0, gx = 0, gy = 0, n_tiles = 0;
  size_t n = 0;   // sums per half: rows x width x 3
  unsigned long long* h[2] = {nullptr, nullptr};
  uint32_t* counts = nullptr;
  int* list[2] = {nullptr, nullptr};
  unsigned* state = nullptr;    // device u32[4]
  unsigned* pinned = nullptr;   // host u32[2]
  hipEvent_t ev = nullptr;
  mutable std::mutex mu;
  int step = 0, cur = 0, gen = 0;
  bool pending = false;   // an evaluation's read-back is in flight
  int n_active = 0;
  int64_t px_active = 0, samples = 0;
};

static const char* adapt_opts_error(const rt_adapt_opts& o) {
  if (o.step_spp < 1) return "step_spp < 1";
  const int64_t two = 2 * static_cast<int64_t>(o.step_spp);
  if (o.min_spp <= 0 || o.min_spp % two != 0) return "min_spp is no positive multiple of 2 * step_spp";
  if (o.max_spp <= 0 || o.max_spp % two != 0) return "max_spp is no positive multiple of 2 * step_spp";
  if (o.min_spp > o.max_spp) return "min_spp > max_spp";
  if (o.max_spp > RT_MAX_SPP) return "max_spp > RT_MAX_SPP";
  if (o.tol_q16 > 65536u) return "tol_q16 > 65536";
  return nullptr;
}

static void adapt_release(rt_adapt* ad) {
  (void)hipSetDevice(ad->device);
  for (int k = 0; k < 2; ++k) {
    if (ad->h[k]) (void)hipFree(ad->h[k]);
    if (ad->list[k]) (void)hipFree(ad->list[k]);
  }
  if (ad->counts) (void)hipFree(ad->counts);
  if (ad->state) (void)hipFree(ad->state);
  if (ad->pinned) (void)hipHostFree(ad->pinned);
  if (ad->ev) (void)hipEventDestroy(ad->ev);
  delete ad;
}

// step 0, every tile active, sums and counts zero: enqueued on stream
static hipError_t adapt_reset(rt_adapt* ad, hipStream_t stream) {
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k)
    e = static_cast<hipError_t>(fill_async(ad->h[k], 0, ad->n * sizeof(unsigned long long), stream));
  if (e != hipSuccess) return e;
  int* list = ad->list[0];
  uint32_t* counts = ad->counts;
  unsigned* state = ad->state;
  int n = ad->n_tiles;
  void* args[] = {&list, &counts, &state, &n};
  e = hipLaunchKernel(reinterpret_cast<const void*>(&adapt_reset_kernel), dim3(static_cast<unsigned>((n + 255) / 256)),
                      dim3(256), args, 0, stream);
  ad->step = ad->cur = ad->gen = 0;
  ad->pending = false;
  ad->n_active = ad->n_tiles;
  ad->px_active = static_cast<int64_t>(ad->rows) * ad->shape.width;
  ad->samples = 0;
  return e;
}

extern "C" int rt_adapt_create(const rt_dscene* ds, const rt_params* shape, const rt_adapt_opts* opts,
                               rt_adapt** out) {
  clear_error();
  if (out) *out = nullptr;
  if (!shape || !opts || !out) return set_error(RT_E_ARG, "rt_adapt_create: NULL argument");
  if (const char* why = adapt_opts_error(*opts)) return set_error(RT_E_ARG, std::string("rt_adapt_create: ") + why);
  if (!ds) return set_error(RT_E_ARG, "rt_adapt_create: NULL argument");
  const int rows = rows_out(*shape);
  if (shape->width <= 0 || shape->height <= 0 || rows <= 0)
    return set_error(RT_E_ARG, "rt_adapt_create: bad width/height/row selection");
  const int64_t tiles = static_cast<int64_t>((shape->width + kTile - 1) / kTile) * ((rows + kTile - 1) / kTile);
  // (the resolve's grid has a block row per frame row; the pixel count is a u32)
  if (rows > 65535 || tiles > INT_MAX / kSplitMax || static_cast<int64_t>(rows) * shape->width > 0xffffffffll)
    return set_error(RT_E_ARG, "rt_adapt_create: frame too large (more than 65535 rows)");
  HIP_TRY(hipSetDevice(ds->device));
  rt_adapt* ad = new rt_adapt;
  ad->device = ds->device;
  ad->shape = accum_shape(*shape);
  ad->opts = *opts;
  ad->rows = rows;
  ad->gx = (shape->width + kTile - 1) / kTile;
  ad->gy = (rows + kTile - 1) / kTile;
  ad->n_tiles = static_cast<int>(tiles);
  ad->n = static_cast<size_t>(rows) * shape->width * 3;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = hipMalloc(&ad->h[k], ad->n * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&ad->list[k], ad->n_tiles * sizeof(int));
  }
  if (e == hipSuccess) e = hipMalloc(&ad->counts, ad->n_tiles * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&ad->state, 4 * sizeof(unsigned));
  if (e == hipSuccess) e = hipHostMalloc(&ad->pinned, 2 * sizeof(unsigned));
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ad->ev, hipEventDisableTiming);
  // ready before the call returns: the first step may come on any stream
  if (e == hipSuccess) e = adapt_reset(ad, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    adapt_release(ad);
    return hip_fail(e, "rt_adapt_create");
  }
  *out = ad;
  return RT_OK;
}

extern "C" int rt_adapt_free(rt_adapt* ad) {
  if (!ad) return RT_OK;
  if (ad->pending) (void)hipEventSynchronize(ad->ev);   // (the copy into `pinned`)
  adapt_release(ad);
  return RT_OK;
}

extern "C" int rt_adapt_clear(rt_adapt* ad, void* hip_stream) {
  clear_error();
  if (!ad) return set_error(RT_E_ARG, "rt_adapt_clear: NULL argument");
  std::lock_guard<std::mutex> lk(ad->mu);
  HIP_TRY(hipSetDevice(ad->device));
  if (ad->pending) HIP_TRY(hipEventSynchronize(ad->ev));
  HIP_TRY(adapt_reset(ad, static_cast<hipStream_t>(hip_stream)));
  return RT_OK;
}

// the evaluation in flight, if any: wait for it and take its two numbers
static int adapt_settle(rt_adapt* ad) {
  if (!ad->pending) return RT_OK;
  HIP_TRY(hipEventSynchronize(ad->ev));
  ad->pending = false;
  ad->n_active = static_cast<int>(ad->pinned[0]);
  ad->px_active = static_cast<int64_t>(ad->pinned[1]);
  return RT_OK;
}

extern "C" int rt_adapt_step(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_adapt* ad,
                             uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!ds || !c || !p || !ad) return set_error(RT_E_ARG, "rt_adapt_step: NULL argument");
  if (ds->device != ad->device)
    return set_error(RT_E_ARG, "rt_adapt_step: the scene is on device " + std::to_string(ds->device) +
                                   ", the adaptive frame on device " + std::to_string(ad->device));
  if (!same_shape(accum_shape(*p), ad->shape))
    return set_error(RT_E_ARG, "rt_adapt_step: width/height/row selection differ from the adaptive frame's");
  std::lock_guard<std::mutex> lk(ad->mu);
  const rt_adapt_opts& o = ad->opts;
  if (p->sample_begin < 0 || static_cast<int64_t>(p->sample_begin) + o.max_spp > INT_MAX)
    return set_error(RT_E_ARG, "rt_adapt_step: sample_begin + max_spp passes 2^31 - 1");
  HIP_TRY(hipSetDevice(ad->device));
  if (const int rc = adapt_settle(ad)) return rc;
  if (ad->n_active == 0) return 0;
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  rt_params q = *p;
  q.spp = o.step_spp;
  q.sample_begin = p->sample_begin + ad->step * o.step_spp;
  const int traced = ad->n_active;
  const int rc = launch_impl(ds, c, &q, nullptr, d_counters, hip_stream, ad->h[ad->step & 1], "rt_adapt_step",
                             ad->list[ad->cur], traced);
  if (rc != RT_OK) return rc;
  ad->samples += ad->px_active * o.step_spp;
  ++ad->step;
  // behind the trace: the tiles' new count, and after an odd step that
  // reached min_spp the rule (at max_spp every tile leaves untested)
  uint32_t count = static_cast<uint32_t>(ad->step) * static_cast<uint32_t>(o.step_spp);
  const bool even_halves = (ad->step & 1) == 0;
  const bool at_cap = even_halves && count >= static_cast<uint32_t>(o.max_spp);
  int decide = even_halves && !at_cap && count >= static_cast<uint32_t>(o.min_spp);
  const unsigned long long *h0 = ad->h[0], *h1 = ad->h[1];
  int width = ad->shape.width, rows = ad->rows, tiles_x = ad->gx, n_active = traced;
  const int* active = ad->list[ad->cur];
  int* next = ad->list[ad->cur ^ 1];
  unsigned* state = ad->state + 2 * (ad->gen & 1);
  unsigned* state_next = decide ? ad->state + 2 * ((ad->gen + 1) & 1) : nullptr;
  uint32_t* counts = ad->counts;
  uint32_t tol = o.tol_q16;
  void* args[] = {&h0, &h1, &width, &rows, &tiles_x, &active, &n_active, &next, &state, &state_next, &counts,
                  &count, &tol, &decide};
  HIP_TRY(hipLaunchKernel(reinterpret_cast<const void*>(&adapt_eval_kernel),
                          dim3(static_cast<unsigned>((n_active + kEvalWaves - 1) / kEvalWaves)), dim3(64 * kEvalWaves),
                          args, 0, stream));
  if (decide) {
    HIP_TRY(hipMemcpyAsync(ad->pinned, state, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(ad->ev, stream));
    ad->pending = true;
    ad->cur ^= 1;
    ++ad->gen;
  } else if (at_cap) {
    ad->n_active = 0;
    ad->px_active = 0;
  }
  return traced;
}

extern "C" int rt_adapt_active(const rt_adapt* ad) {
  if (!ad) return 0;
  std::lock_guard<std::mutex> lk(ad->mu);
  return ad->n_active;
}

extern "C" int64_t rt_adapt_samples(const rt_adapt* ad) {
  if (!ad) return 0;
  std::lock_guard<std::mutex> lk(ad->mu);
  return ad->samples;
}

static int adapt_resolve(const rt_adapt* ad, int flags, float* d_f, uint8_t* d_u8, void* hip_stream,
                         const char* who) {
  clear_error();
  if (!ad || (!d_f && !d_u8)) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  if ((flags & ~(RT_FLAG_REALM | RT_FLAG_STREAMED | RT_FLAG_REJECTION_SAMPLERS)) != 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad flags");
  static const QThr thr = [] {
    QThr t;
    std::memcpy(t.t, quantize_thresholds(), sizeof t.t);
    return t;
  }();
  HIP_TRY(hipSetDevice(ad->device));
  const unsigned long long *h0 = ad->h[0], *h1 = ad->h[1];
  const uint32_t* counts = ad->counts;
  int width = ad->shape.width, tiles_x = ad->gx, realm = (flags & RT_FLAG_REALM) ? 1 : 0;
  QThr q = thr;
  const unsigned bx = static_cast<unsigned>(std::max(1, std::min((width * 3 / 2 + 255) / 256, 64)));
  void* args[] = {&h0, &h1, &counts, &width, &tiles_x, &realm, &d_f, &d_u8, &q};
  // (the rows are the grid's y: rt_adapt_create admits at most 65535)
  HIP_TRY(hipLaunchKernel(reinterpret_cast<const void*>(&adapt_resolve_kernel),
                          dim3(bx, static_cast<unsigned>(ad->rows)), dim3(256), args, 0,
                          static_cast<hipStream_t>(hip_stream)));
  return RT_OK;
}

extern "C" int rt_adapt_resolve(const rt_adapt* ad, int flags, float* d_out, void* hip_stream) {
  return adapt_resolve(ad, flags, d_out, nullptr, hip_stream, "rt_adapt_resolve");
}

extern "C" int rt_adapt_resolve_u8(const rt_adapt* ad, int flags, uint8_t* d_out, void* hip_stream) {
  return adapt_resolve(ad, flags, nullptr, d_out, hip_stream, "rt_adapt_resolve_u8");
}

extern "C" int rt_adapt_counts(const rt_adapt* ad, uint32_t* host_counts, void* hip_stream) {
  clear_error();
  if (!ad || !host_counts) return set_error(RT_E_ARG, "rt_adapt_counts: NULL argument");
  HIP_TRY(hipSetDevice(ad->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_counts, ad->counts, ad->n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_adapt_read(const rt_adapt* ad, uint64_t* host_sums0, uint64_t* host_sums1, void* hip_stream) {
  clear_error();
  if (!ad || !host_sums0 || !host_sums1) return set_error(RT_E_ARG, "rt_adapt_read: NULL argument");
  HIP_TRY(hipSetDevice(ad->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_sums0, ad->h[0], ad->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(host_sums1, ad->h[1], ad->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

// ---- first-hit features: albedo, normal, depth, coverage (rt.h, first_hit.h) ----
// Per pixel six 64-bit sums (albedo rgb, normal xyz, 2^-24 units), a u32 hit
// count and the nearest hit distance as float bits, on the scene's device; the
// samples per pixel they hold on the host side, as rt_accum keeps them.
struct rt_feat {
  int device = 0;
  rt_params shape{};   // width, height and the row selection (row_tile resolved)
  size_t n_px = 0;     // rows_out x width
  unsigned long long* sums = nullptr;   // n_px x 6
  unsigned* hits = nullptr;             // n_px
  unsigned* depth = nullptr;            // n_px, float bits (+inf: no hit yet)
  mutable std::mutex mu;
  int64_t samples = 0;
};

// Where a feature launch on ds takes its bodies from, classed as
// resolve_variant classes the path kernel's variants: the selector's scan
// variants (5, the diagnostic 1-10) and a tree too deep for the stack give the
// linear scan; 12, or a tree image beyond the LDS budget, the tree in global
// memory; everything else the tree in LDS.  The tree is the 4-body-leaf one
// (tree[1]): half the nodes of the 2-body tree, and int body indices (the
// 8-body tree's are u16).  Budget: blob + stack rows within 160 KB / 5 less
// the kernel's 3.6 KB of static LDS, five workgroups per CU.
constexpr size_t kFeatLdsBudget = 160 * 1024 / 5 - 4096;
static int feat_stack_rows(const DTree& t) { return t.depth + 1; }
static size_t feat_stack_bytes(const DTree& t) { return static_cast<size_t>(feat_stack_rows(t)) * kFeatThreads * 2; }
static int feat_source(const rt_dscene& ds, int vsel) {
  const int v = resolve_variant(ds, vsel);
  const DTree& t = ds.tree[1];
  if (v < 11 || t.depth + 2 > kBvhStack) return FEAT_SCAN;
  if (v == 12 || static_cast<size_t>(t.blob_f4) * 16 + feat_stack_bytes(t) > kFeatLdsBudget) return FEAT_GLOBAL;
  return FEAT_LDS;
}
static const void* feat_fn(int src) {
  return src == FEAT_LDS      ? reinterpret_cast<const void*>(&feat_kernel<FEAT_LDS>)
         : src == FEAT_GLOBAL ? reinterpret_cast<const void*>(&feat_kernel<FEAT_GLOBAL>)
                              : reinterpret_cast<const void*>(&feat_kernel<FEAT_SCAN>);
}
static size_t feat_lds(const rt_dscene& ds, int src) {
  const DTree& t = ds.tree[1];
  return src == FEAT_SCAN ? 0 : feat_stack_bytes(t) + (src == FEAT_LDS ? static_cast<size_t>(t.blob_f4) * 16 : 0);
}

// words of a feature buffer set to v (fill_kernel takes any word: +inf's bits)
static hipError_t feat_fill(void* p, uint32_t v, size_t words, hipStream_t stream) {
  uint32_t* w = static_cast<uint32_t*>(p);
  size_t n = words;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 2048));
  void* args[] = {&w, &v, &n};
  return hipLaunchKernel(reinterpret_cast<const void*>(&fill_kernel), dim3(static_cast<unsigned>(blocks)), dim3(256),
                         args, 0, stream);
}
static hipError_t feat_reset(rt_feat* f, hipStream_t stream) {
  hipError_t e = feat_fill(f->sums, 0u, f->n_px * 12, stream);
  if (e == hipSuccess) e = feat_fill(f->hits, 0u, f->n_px, stream);
  if (e == hipSuccess) e = feat_fill(f->depth, 0x7f800000u, f->n_px, stream);
  return e;
}

extern "C" int rt_feat_create(const rt_dscene* ds, const rt_params* shape, rt_feat** out) {
  clear_error();
  if (!ds || !shape || !out) return set_error(RT_E_ARG, "rt_feat_create: NULL argument");
  *out = nullptr;
  const int rows = rows_out(*shape);
  if (shape->width <= 0 || shape->height <= 0 || rows <= 0)
    return set_error(RT_E_ARG, "rt_feat_create: bad width/height/row selection");
  HIP_TRY(hipSetDevice(ds->device));
  rt_feat* f = new rt_feat;
  f->device = ds->device;
  f->shape = accum_shape(*shape);
  f->n_px = static_cast<size_t>(rows) * shape->width;
  // cleared before the call returns: the first pass may come on any stream
  hipError_t e = hipMalloc(&f->sums, f->n_px * 6 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(&f->hits, f->n_px * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc(&f->depth, f->n_px * sizeof(unsigned));
  if (e == hipSuccess) e = feat_reset(f, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    rt_feat_free(f);
    return hip_fail(e, "rt_feat_create");
  }
  *out = f;
  return RT_OK;
}

extern "C" int rt_feat_free(rt_feat* f) {
  if (!f) return RT_OK;
  (void)hipSetDevice(f->device);
  if (f->sums) (void)hipFree(f->sums);
  if (f->hits) (void)hipFree(f->hits);
  if (f->depth) (void)hipFree(f->depth);
  delete f;
  return RT_OK;
}

extern "C" int rt_feat_clear(rt_feat* f, void* hip_stream) {
  clear_error();
  if (!f) return set_error(RT_E_ARG, "rt_feat_clear: NULL argument");
  std::lock_guard<std::mutex> lk(f->mu);
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(feat_reset(f, static_cast<hipStream_t>(hip_stream)));
  f->samples = 0;
  return RT_OK;
}

extern "C" int64_t rt_feat_samples(const rt_feat* f) {
  if (!f) return 0;
  std::lock_guard<std::mutex> lk(f->mu);
  return f->samples;
}

extern "C" int rt_launch_feat(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_feat* f,
                              uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!ds || !c || !p || !f) return set_error(RT_E_ARG, "rt_launch_feat: NULL argument");
  if (p->width <= 0 || p->height <= 0 || p->spp < 0 || p->spp > RT_MAX_SPP ||
      (p->flags & ~(RT_FLAG_REALM | RT_FLAG_STREAMED | RT_FLAG_REJECTION_SAMPLERS)) != 0)
    return set_error(RT_E_ARG, "rt_launch_feat: bad width/height/spp/flags");
  if (ds->device != f->device)
    return set_error(RT_E_ARG, "rt_launch_feat: the scene is on device " + std::to_string(ds->device) +
                                   ", the feature buffers on device " + std::to_string(f->device));
  if (!same_shape(accum_shape(*p), f->shape))
    return set_error(RT_E_ARG, "rt_launch_feat: width/height/row selection differ from the feature buffers'");
  std::lock_guard<std::mutex> lk(f->mu);
  if (p->spp > 0 && f->samples + p->spp > kAccumMaxSamples)
    return set_error(RT_E_ARG, "rt_launch_feat: more than 2^32 - 1 samples per pixel");
  if (p->spp == 0) return RT_OK;
  const int rows = rows_out(*p);
  HIP_TRY(hipSetDevice(ds->device));
  const int src = feat_source(*ds, g_variant.load());
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
  std::memcpy(a.cam + 0, c->center, 12);
  std::memcpy(a.cam + 3, c->p00, 12);
  std::memcpy(a.cam + 6, c->du, 12);
  std::memcpy(a.cam + 9, c->dv, 12);
  std::memcpy(a.cam + 12, c->disk_u, 12);
  std::memcpy(a.cam + 15, c->disk_v, 12);
  a.defocus = c->defocus ? 1 : 0;
  a.sampler = (p->flags & RT_FLAG_REJECTION_SAMPLERS) ? 0 : (RT_SAMPLER_SPHERE | RT_SAMPLER_DISK);
  a.n = ds->n;
  a.width = p->width;
  a.rows_out = rows;
  a.row_begin = p->row_begin;
  a.row_tile = p->row_tile > 0 ? p->row_tile : 8;
  a.tile_first = p->tile_first;
  a.tile_step = p->tile_step;
  a.tiles_x = (p->width + kTile - 1) / kTile;
  a.spp = p->spp;
  a.sample_begin = p->sample_begin;
  a.key = seed_key(p->seed);
  a.sums = f->sums;
  a.hits = f->hits;
  a.depth = f->depth;
  a.counters = reinterpret_cast<unsigned long long*>(d_counters);
  const int gy = (rows + kTile - 1) / kTile;
  void* args[] = {&a};
  HIP_TRY(hipLaunchKernel(feat_fn(src), dim3(static_cast<unsigned>(a.tiles_x * gy)), dim3(kFeatThreads), args,
                          feat_lds(*ds, src), static_cast<hipStream_t>(hip_stream)));
  f->samples += p->spp;
  return RT_OK;
}

extern "C" int rt_feat_resolve(const rt_feat* f, float* d_out, void* hip_stream) {
  clear_error();
  if (!f || !d_out) return set_error(RT_E_ARG, "rt_feat_resolve: NULL argument");
  int64_t count;
  {
    std::lock_guard<std::mutex> lk(f->mu);
    count = f->samples;
  }
  HIP_TRY(hipSetDevice(f->device));
  const unsigned long long* sums = f->sums;
  const unsigned *hits = f->hits, *depth = f->depth;
  size_t n_px = f->n_px;
  float nf = static_cast<float>(count > 0 ? count : 1);   // RN(float(n))
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((n_px + 255) / 256, 4096));
  void* args[] = {&sums, &hits, &depth, &n_px, &nf, &d_out};
  HIP_TRY(hipLaunchKernel(reinterpret_cast<const void*>(&feat_resolve_kernel), dim3(static_cast<unsigned>(blocks)),
                          dim3(256), args, 0, static_cast<hipStream_t>(hip_stream)));
  return RT_OK;
}

extern "C" int rt_feat_read(const rt_feat* f, int64_t* host_sums, uint32_t* host_hits, float* host_depth,
                            void* hip_stream) {
  clear_error();
  if (!f || !host_sums || !host_hits || !host_depth) return set_error(RT_E_ARG, "rt_feat_read: NULL argument");
  HIP_TRY(hipSetDevice(f->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_sums, f->sums, f->n_px * 6 * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(host_hits, f->hits, f->n_px * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(host_depth, f->depth, f->n_px * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_feat_add(rt_feat* f, const int64_t* host_sums, const uint32_t* host_hits, const float* host_depth,
                           int64_t samples, void* hip_stream) {
  clear_error();
  if (!f || !host_sums || !host_hits || !host_depth) return set_error(RT_E_ARG, "rt_feat_add: NULL argument");
  std::lock_guard<std::mutex> lk(f->mu);
  if (samples < 0 || samples > kAccumMaxSamples || f->samples + samples > kAccumMaxSamples)
    return set_error(RT_E_ARG, "rt_feat_add: samples negative, or more than 2^32 - 1 per pixel in all");
  for (size_t i = 0; i < f->n_px; ++i)   // (a depth is a positive distance or +inf: the minimum runs on the bits)
    if (!(host_depth[i] > 0.0f)) return set_error(RT_E_ARG, "rt_feat_add: a depth is not a positive distance or +inf");
  HIP_TRY(hipSetDevice(f->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  // one staging block: sums | hits | depth (freed when the call returns)
  const size_t sb = f->n_px * 6 * sizeof(uint64_t), wb = f->n_px * sizeof(uint32_t);
  char* stage = nullptr;
  HIP_TRY(hipMalloc(&stage, sb + 2 * wb));
  hipError_t e = hipMemcpyAsync(stage, host_sums, sb, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(stage + sb, host_hits, wb, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(stage + sb + wb, host_depth, wb, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    unsigned long long* sums = f->sums;
    unsigned *hits = f->hits, *depth = f->depth;
    const unsigned long long* as = reinterpret_cast<const unsigned long long*>(stage);
    const unsigned* ah = reinterpret_cast<const unsigned*>(stage + sb);
    const unsigned* ad = reinterpret_cast<const unsigned*>(stage + sb + wb);
    size_t n_px = f->n_px;
    const size_t blocks = std::max<size_t>(1, std::min<size_t>((n_px + 255) / 256, 4096));
    void* args[] = {&sums, &hits, &depth, &as, &ah, &ad, &n_px};
    e = hipLaunchKernel(reinterpret_cast<const void*>(&feat_add_kernel), dim3(static_cast<unsigned>(blocks)), dim3(256),
                        args, 0, stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(stage);
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
  const int src = feat_source(*ds, g_variant.load());
  const size_t lds = feat_lds(*ds, src);
  int blocks = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, feat_fn(src), kFeatThreads, lds));
  hipFuncAttributes fa{};
  HIP_TRY(hipFuncGetAttributes(&fa, feat_fn(src)));
  out4[0] = blocks;
  out4[1] = fa.numRegs;
  out4[2] = static_cast<int>(lds + fa.sharedSizeBytes);
  out4[3] = src;
  return RT_OK;
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
  HIP_TRY(hipFuncGetAttributes(&fa, variant_table(16).fn));
  const auto t2 = Clk::now();
  constexpr size_t kProbe = 64 * 1024;
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, kProbe));
  hipError_t e = static_cast<hipError_t>(fill_async(d, 0, kProbe, nullptr));
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  const auto t3 = Clk::now();
  std::vector<unsigned char> host(kProbe);
  if (e == hipSuccess) e = hipMemcpy(host.data(), d, kProbe, hipMemcpyDeviceToHost);
  const auto t4 = Clk::now();
  (void)hipFree(d);
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
// device that ran a stats launch.
extern "C" int rt_debug_stats(uint64_t* out32) {
  clear_error();
  if (!out32) return set_error(RT_E_ARG, "rt_debug_stats: NULL");
  for (int i = 0; i < kDbg; ++i) out32[i] = 0;
  std::lock_guard<std::mutex> lk(g_dbg_mu);
  for (int d = 0; d < kDbgDevices; ++d) {
    if (!g_dbg[d]) continue;
    uint64_t v[kDbg];
    HIP_TRY(hipSetDevice(d));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(v, g_dbg[d], sizeof v, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(g_dbg[d], 0, sizeof v));
    for (int i = 0; i < kDbg; ++i) out32[i] += v[i];
  }
  return RT_OK;
}

// Steals of the launches on (ds, stream) since the last call: out2 =
// {steals, samples stolen}; waits for the stream, then clears them.
extern "C" int rt_steal_stats(const rt_dscene* ds, void* hip_stream, uint64_t* out2) {
  clear_error();
  if (!ds || !out2) return set_error(RT_E_ARG, "rt_steal_stats: NULL argument");
  out2[0] = out2[1] = 0;
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  std::lock_guard<std::mutex> lk(ds->sched.mu);
  for (int k = 0; k < ds->sched.used; ++k) {
    const Schedule& e = ds->sched.s[k];
    if (e.stream != stream || !e.stealc) continue;
    HIP_TRY(hipSetDevice(ds->device));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(out2, e.stealc, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(e.stealc, 0, 2 * sizeof(uint64_t)));
  }
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
  for (int k = 0; k < ds->sched.used; ++k) {
    Schedule& e = ds->sched.s[k];
    if (e.stream != stream || !e.xq_n) continue;
    HIP_TRY(hipSetDevice(ds->device));
    HIP_TRY(hipStreamSynchronize(stream));
    unsigned n[2] = {0, 0};
    HIP_TRY(hipMemcpy(n, e.xq_n, sizeof n, hipMemcpyDeviceToHost));
    out2[0] = e.xq_launches;
    out2[1] = n[0];
    e.xq_launches = 0;
  }
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
