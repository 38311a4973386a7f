// trace.hip — the product library's gfx950 code object and host side: the
// shipped kernel's instantiations (trace_kernel.h: the default BVH walk in its
// two LDS images and its fallbacks), the schedule / split / quantise / fill
// kernels, the accumulator's resolve / add kernels, the adaptive sampler's
// evaluation / resolve kernels, and rt_scene_upload / rt_launch /
// rt_launch_accum / rt_adapt_step and the rt_accum and rt_adapt entries.  The A/B scans, the
// direction-coherent waves and the statistics builds live in trace_diag.hip
// (librtclj_diag.so only).  DESIGN.md §3.  The first-hit feature pass
// (first_hit.h: feat_kernel, feat_resolve_kernel) and the rt_feat entries are
// here too.  Which variant a launch runs and the LDS it needs
// is variant_policy.h's (pure functions, checked on the CPU); the device
// buffers the host side owns are dev_buf.h's DevBuf.  The denoiser's kernels
// (denoise.h) and the rt_denoiser entries, then temporal accumulation's kernel
// (temporal.h) and the rt_temporal entries close the file;
// the body-id pass (body_ids.h, rt_launch_ids) stands behind the feature pass
// and the motion-aware step beside rt_temporal_step;
// rt_scene_update and the refit kernel (bvh_refit.h) are the last section
// (DESIGN.md §3.11).  The sample budget (budget.h's plan kernels, the rt_budget
// entries, rt_temporal_probe and rt_temporal_step_budget) stands behind the
// rt_temporal entries.
#include "trace_kernel.h"
#define RT_FIRST_HIT_KERNEL
#include "first_hit.h"
#define RT_DENOISE_KERNEL
#include "denoise.h"
#define RT_TEMPORAL_KERNEL
#include "temporal.h"
#define RT_BUDGET_KERNEL
#include "budget.h"
#define RT_BODY_IDS_KERNEL
#include "body_ids.h"
#define RT_REFIT_KERNEL
#include "bvh_refit.h"
#include "variant_policy.h"
#include "dev_buf.h"

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
#include <utility>
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

// rt_adapt_resolve_half: one half's sums as a frame, resolve_kernel's
// conversion with half the count of the element's tile (each half holds half
// the tile's samples).  A thread per element, grid-stride.
__global__ __launch_bounds__(256) void adapt_half_kernel(const unsigned long long* __restrict__ h,
                                                          const uint32_t* __restrict__ counts, int width,
                                                          int tiles_x, size_t n, int realm, float* __restrict__ out) {
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t e = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; e < n; e += stride) {
    const size_t px = e / 3, y = px / static_cast<size_t>(width), x = px - y * static_cast<size_t>(width);
    const uint32_t c = counts[(y / kTile) * tiles_x + x / kTile] / 2u;
    const float nf = static_cast<float>(c > 0u ? c : 1u);   // RN(float(count / 2))
    const float tot = static_cast<float>(h[e]) * 0x1p-24f;
    out[e] = realm ? tot * (1.0f / nf) : tot / nf;
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
static_assert(policy::kTile == kTile && policy::kPoolPx == kPoolPx && policy::kXBytes == kXBytes &&
                  policy::kFeatThreads == kFeatThreads && static_cast<int>(policy::FEAT_LDS) == FEAT_LDS &&
                  static_cast<int>(policy::FEAT_GLOBAL) == FEAT_GLOBAL && static_cast<int>(policy::FEAT_SCAN) == FEAT_SCAN,
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
    case policy::kCompact: return RT_K(SRC_LDS, SCAN_BVHQ7, false);
    case policy::kCompactW8: return RT_KW(SRC_LDS, SCAN_BVHQ7, false, 8);
    case policy::kCompactW16: return trace_kernel_w16();   // (trace_w16.hip, compiled with its own scheduler flag)
    case policy::kCompactTh4: return RT_KWT(SRC_LDS, SCAN_BVHQ7, false, 4, 4);
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
constexpr int kDbg = 32;
constexpr int kDbgDevices = 64;
static std::mutex g_dbg_mu;
static unsigned long long* g_dbg[kDbgDevices] = {};
static unsigned long long* g_dbgw[kDbgDevices] = {};

}  // namespace rtclj

using namespace rtclj;

static int hip_fail(hipError_t e, const char* what) {
  return set_error(RT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(call)                                  \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return hip_fail(_e, #call);  \
  } while (0)

// A launch of one of this file's kernels: each argument converted to the
// kernel's parameter type at compile time (a narrowing one is an error), then
// the pointer array hipLaunchKernel takes.
template <class... P, class... Args>
static hipError_t enqueue(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args&&... args) {
  static_assert(sizeof...(P) == sizeof...(Args), "enqueue: the kernel's parameter count");
  const auto launch = [&](P... v) {
    void* ptrs[] = {const_cast<void*>(static_cast<const void*>(&v))...};
    return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, lds, stream);
  };
  return launch(P{std::forward<Args>(args)}...);
}
// ... of a variant-table kernel: one KArgs / FeatArgs by value
template <class A>
static hipError_t enqueue(const void* fn, dim3 grid, dim3 block, size_t lds, hipStream_t stream, A& a) {
  void* ptrs[] = {&a};
  return hipLaunchKernel(fn, grid, block, ptrs, lds, stream);
}

// The library's fill: n words of p set to `word` (fill_kernel takes any
// word: +inf's bits for the feature depths)
static hipError_t fill_words(void* p, uint32_t word, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const size_t blocks = std::min<size_t>((n + 255) / 256, 2048);
  return enqueue(fill_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, static_cast<uint32_t*>(p), word, n);
}
template <class T>
static hipError_t fill_zero(const DevBuf<T>& b, size_t n, hipStream_t stream) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  return fill_words(b.p, 0u, n * (sizeof(T) / 4), stream);
}
static const QThr& quantize_table() {
  static const QThr thr = [] {
    QThr t;
    std::memcpy(t.t, quantize_thresholds(), sizeof t.t);
    return t;
  }();
  return thr;
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
// Its methods are rt_launch's stages (below, above launch_impl).
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
  RefitState refit;            // rt_scene_update's
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

// Tile sharing, A/B knobs read at every launch:
// RTCLJ_STEAL=0 (off: the static sample split for launches of few tiles, as
// before), RTCLJ_THIEVES (helper workgroups per workgroup slot of the
// device), RTCLJ_STEAL_MIN (unclaimed samples a tile needs for a helper to join)
static int env_int(const char* name, int dflt, int lo) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::atoi(e)) : dflt;
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

// what the selection policy (variant_policy.h) reads of a scene, of a frame
static policy::Scene scene_info(const rt_dscene& ds) {
  policy::Scene s{};
  for (int k = 0; k < 3; ++k) s.tree[k] = policy::Tree{ds.tree[k].n_nodes, ds.tree[k].depth, ds.tree[k].blob_f4};
  s.n_pad = ds.n_pad;
  s.unit_albedo = ds.unit_albedo;
  return s;
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

// The HIP occupancy query on a kernel at a workgroup size and dynamic LDS:
// out4[0..2] = {workgroups per CU, VGPRs per lane, LDS bytes per workgroup}
static int occupancy_report(const void* fn, int threads, size_t lds, int* out4) {
  int blocks = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, threads, lds));
  hipFuncAttributes fa{};
  HIP_TRY(hipFuncGetAttributes(&fa, fn));
  out4[0] = blocks;
  out4[1] = fa.numRegs;
  out4[2] = static_cast<int>(lds + fa.sharedSizeBytes);
  return RT_OK;
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
// a launch's frame arguments (rt_launch, rt_launch_accum, rt_adapt_step, rt_launch_feat)
static int check_frame_args(const char* who, const rt_params& p) {
  if (p.width <= 0 || p.height <= 0 || p.spp < 0 || p.spp > RT_MAX_SPP ||
      (p.flags & ~(RT_FLAG_REALM | RT_FLAG_STREAMED | RT_FLAG_REJECTION_SAMPLERS)) != 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad width/height/spp/flags");
  return RT_OK;
}

// The camera, sampler, seed key and row selection of a launch: the fields
// KArgs and FeatArgs share by name
template <class A>
static void pack_frame(A& a, const rt_camera& c, const rt_params& p, int rows) {
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

// The variant a launch runs: its number, traits and kernels
struct Kernel {
  int vsel;
  policy::Traits t;
  const void* fn;
  const void* sweep;
};
// ... chosen for (ds, p), and its tree and stack bound to the arguments
static int bind_variant(const char* who, const rt_dscene& ds, const rt_params& p, KArgs& a, Kernel* out) {
  int vsel = launch_variant(ds, p);
  if (variant_traits(vsel).walk == policy::WALK_SORTED && p.max_depth > 1023)
    vsel = policy::kFull4;   // (a path's depth left: 10 bits in the exchange)
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
static int launch_impl(const rt_dscene* ds, const rt_camera* c, const rt_params* p, float* d_out,
                       uint64_t* d_counters, void* hip_stream, unsigned long long* acc_sums,
                       const char* who = "rt_launch", const int* active = nullptr, int n_active = 0) {
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
  const int n_tiles = active ? n_active : gx * gy;
  a.tiles_x = gx;
  if (const int rc = bind_debug(ds->device, v, a)) return rc;
  size_t lds = 0;
  if (const int rc = bind_lds(*ds, v, &lds)) return rc;
  // the stream's entry: adaptive schedule and split partial sums
  Schedule* sch = nullptr;
  std::unique_lock<std::mutex> sched_lock;
  if (!active) {
    sched_lock = std::unique_lock<std::mutex>(ds->sched.mu);
    sch = ds->sched.entry(stream);
  }
  const bool steal = sch && env_int("RTCLJ_STEAL", 1, 0) != 0 && !v.t.stats && v.t.walk != policy::WALK_SORTED;
  const int split = ((sch || acc_sums) && p->spp > 1) ? launch_split(*ds, v, lds, n_tiles, *p) : 1;
  // (an accumulating pass: every unit's sums go to part[])
  const int n_whole = (split > 1 || acc_sums) ? 0 : n_tiles;
  a.split = split;
  a.n_whole = n_whole;
  a.rt_magic = magic64(a.row_tile);
  const int64_t n_units64 = n_whole + static_cast<int64_t>(n_tiles - n_whole) * split;
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
// a create's shape: *rows = its output rows (> 0)
static int frame_rows(const char* who, const rt_params& shape, int* rows) {
  *rows = rows_out(shape);
  if (shape.width <= 0 || shape.height <= 0 || *rows <= 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad width/height/row selection");
  return RT_OK;
}
// a pass of p on ds into b (`noun`): the same device, the same shape
static int check_match(const char* who, const char* noun, const FrameBuf& b, const rt_dscene& ds, const rt_params& p) {
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
static int check_pass(const char* who, const char* noun, const FrameBuf& b, const rt_dscene& ds, const rt_params& p) {
  if (const int rc = check_match(who, noun, b, ds, p)) return rc;
  if (p.spp > 0 && b.samples + p.spp > kAccumMaxSamples)
    return set_error(RT_E_ARG, std::string(who) + ": more than 2^32 - 1 samples per pixel");
  return RT_OK;
}
// sums of `samples` samples per pixel added from the host (the caller holds b.mu)
static int check_add(const char* who, const FrameBuf& b, int64_t samples) {
  if (samples < 0 || samples > kAccumMaxSamples || b.samples + samples > kAccumMaxSamples)
    return set_error(RT_E_ARG, std::string(who) + ": samples negative, or more than 2^32 - 1 per pixel in all");
  return RT_OK;
}
static int64_t frame_samples(const FrameBuf* b) {
  if (!b) return 0;
  std::lock_guard<std::mutex> lk(b->mu);
  return b->samples;
}
// a create's new buffer object for `shape` on ds's device, which is made current
template <class B>
static int frame_new(const rt_dscene& ds, const rt_params& shape, B** b) {
  HIP_TRY(hipSetDevice(ds.device));
  *b = new B;
  (*b)->device = ds.device;
  (*b)->shape = accum_shape(shape);
  return RT_OK;
}
// ... handed out once its allocations and first fills (e) are done: the first
// pass may come on any stream
template <class B>
static int frame_created(const char* who, B* b, hipError_t e, B** out) {
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    delete b;
    return hip_fail(e, who);
  }
  *out = b;
  return RT_OK;
}
template <class B>
static int frame_free(B* b) {
  if (!b) return RT_OK;
  (void)hipSetDevice(b->device);
  delete b;
  return RT_OK;
}
static int check_resolve_flags(const char* who, int flags) {
  if ((flags & ~(RT_FLAG_REALM | RT_FLAG_STREAMED | RT_FLAG_REJECTION_SAMPLERS)) != 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad flags");
  return RT_OK;
}

// ---- progressive rendering: the accumulator (rt.h) ------------------------
// The frame's integer sums outlive the launches: rows x width x 3 u64 on the
// scene's device.  mu also orders the one staging buffer of rt_accum_add.
struct rt_accum : FrameBuf {
  size_t n = 0;   // sums: rows_out x width x 3
  DevBuf<unsigned long long> sums;
  DevBuf<unsigned long long> stage;   // rt_accum_add's copy of the caller's sums (n, on first use)
};

extern "C" int rt_accum_create(const rt_dscene* ds, const rt_params* shape, rt_accum** out) {
  clear_error();
  if (!ds || !shape || !out) return set_error(RT_E_ARG, "rt_accum_create: NULL argument");
  *out = nullptr;
  int rows = 0;
  if (const int rc = frame_rows("rt_accum_create", *shape, &rows)) return rc;
  rt_accum* acc = nullptr;
  if (const int rc = frame_new(*ds, *shape, &acc)) return rc;
  acc->n = static_cast<size_t>(rows) * shape->width * 3;
  hipError_t e = acc->sums.alloc(acc->n);
  if (e == hipSuccess) e = fill_zero(acc->sums, acc->n, nullptr);
  return frame_created("rt_accum_create", acc, e, out);
}

extern "C" int rt_accum_free(rt_accum* acc) { return frame_free(acc); }

extern "C" int rt_accum_clear(rt_accum* acc, void* hip_stream) {
  clear_error();
  if (!acc) return set_error(RT_E_ARG, "rt_accum_clear: NULL argument");
  std::lock_guard<std::mutex> lk(acc->mu);
  HIP_TRY(hipSetDevice(acc->device));
  HIP_TRY(fill_zero(acc->sums, acc->n, static_cast<hipStream_t>(hip_stream)));
  acc->samples = 0;
  return RT_OK;
}

extern "C" int64_t rt_accum_samples(const rt_accum* acc) { return frame_samples(acc); }

extern "C" int rt_launch_accum(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_accum* acc,
                               uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!ds || !c || !p || !acc) return set_error(RT_E_ARG, "rt_launch_accum: NULL argument");
  std::lock_guard<std::mutex> lk(acc->mu);
  if (const int rc = check_pass("rt_launch_accum", "the accumulator", *acc, *ds, *p)) return rc;
  const int rc = launch_impl(ds, c, p, nullptr, d_counters, hip_stream, acc->sums.p, "rt_launch_accum");
  if (rc == RT_OK) acc->samples += p->spp;
  return rc;
}

static int accum_resolve(const rt_accum* acc, int flags, float* d_f, uint8_t* d_u8, void* hip_stream,
                         const char* who) {
  clear_error();
  if (!acc || (!d_f && !d_u8)) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  if (const int rc = check_resolve_flags(who, flags)) return rc;
  const int64_t count = frame_samples(acc);
  HIP_TRY(hipSetDevice(acc->device));
  const float nf = static_cast<float>(count > 0 ? count : 1);   // RN(float(n))
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((acc->n / 2 + 255) / 256, 4096));
  HIP_TRY(enqueue(resolve_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
                  acc->sums.p, acc->n, nf, (flags & RT_FLAG_REALM) ? 1 : 0, d_f, d_u8, quantize_table()));
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
  HIP_TRY(hipMemcpyAsync(host_sums, acc->sums.p, acc->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_accum_add(rt_accum* acc, const uint64_t* host_sums, int64_t samples, void* hip_stream) {
  clear_error();
  if (!acc || !host_sums) return set_error(RT_E_ARG, "rt_accum_add: NULL argument");
  std::lock_guard<std::mutex> lk(acc->mu);
  if (const int rc = check_add("rt_accum_add", *acc, samples)) return rc;
  HIP_TRY(hipSetDevice(acc->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (!acc->stage) HIP_TRY(acc->stage.alloc(acc->n));
  HIP_TRY(hipMemcpyAsync(acc->stage.p, host_sums, acc->n * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  const size_t blocks = std::min<size_t>((acc->n + 255) / 256, 4096);
  HIP_TRY(enqueue(accum_add_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, acc->sums.p, acc->stage.p,
                  acc->n));
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
// after it counts in.  (samples: over all pixels, not per pixel.)
struct rt_adapt : FrameBuf {
  rt_adapt_opts opts{};
  int rows = 0, gx = 0, gy = 0, n_tiles = 0;
  size_t n = 0;   // sums per half: rows x width x 3
  DevBuf<unsigned long long> h[2];
  DevBuf<uint32_t> counts;
  DevBuf<int> list[2];
  DevBuf<unsigned> state;       // device u32[4]
  unsigned* pinned = nullptr;   // host u32[2]
  hipEvent_t ev = nullptr;
  int step = 0, cur = 0, gen = 0;
  bool pending = false;   // an evaluation's read-back is in flight
  int n_active = 0;
  int64_t px_active = 0;
  ~rt_adapt() {
    if (pinned) (void)hipHostFree(pinned);
    if (ev) (void)hipEventDestroy(ev);
  }
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

// step 0, every tile active, sums and counts zero: enqueued on stream
static hipError_t adapt_reset(rt_adapt* ad, hipStream_t stream) {
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) e = fill_zero(ad->h[k], ad->n, stream);
  if (e != hipSuccess) return e;
  e = enqueue(adapt_reset_kernel, dim3(static_cast<unsigned>((ad->n_tiles + 255) / 256)), dim3(256), 0, stream,
              ad->list[0].p, ad->counts.p, ad->state.p, ad->n_tiles);
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
  int rows = 0;
  if (const int rc = frame_rows("rt_adapt_create", *shape, &rows)) return rc;
  const int64_t tiles = static_cast<int64_t>((shape->width + kTile - 1) / kTile) * ((rows + kTile - 1) / kTile);
  // (the resolve's grid has a block row per frame row; the pixel count is a u32)
  if (rows > 65535 || tiles > INT_MAX / policy::kSplitMax || static_cast<int64_t>(rows) * shape->width > 0xffffffffll)
    return set_error(RT_E_ARG, "rt_adapt_create: frame too large (more than 65535 rows)");
  rt_adapt* ad = nullptr;
  if (const int rc = frame_new(*ds, *shape, &ad)) return rc;
  ad->opts = *opts;
  ad->rows = rows;
  ad->gx = (shape->width + kTile - 1) / kTile;
  ad->gy = (rows + kTile - 1) / kTile;
  ad->n_tiles = static_cast<int>(tiles);
  ad->n = static_cast<size_t>(rows) * shape->width * 3;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = ad->h[k].alloc(ad->n);
    if (e == hipSuccess) e = ad->list[k].alloc(ad->n_tiles);
  }
  if (e == hipSuccess) e = ad->counts.alloc(ad->n_tiles);
  if (e == hipSuccess) e = ad->state.alloc(4);
  if (e == hipSuccess) e = hipHostMalloc(&ad->pinned, 2 * sizeof(unsigned));
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ad->ev, hipEventDisableTiming);
  if (e == hipSuccess) e = adapt_reset(ad, nullptr);
  return frame_created("rt_adapt_create", ad, e, out);
}

extern "C" int rt_adapt_free(rt_adapt* ad) {
  if (ad && ad->pending) (void)hipEventSynchronize(ad->ev);   // (the copy into `pinned`)
  return frame_free(ad);
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
  if (const int rc = check_match("rt_adapt_step", "the adaptive frame", *ad, *ds, *p)) return rc;
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
  const int rc = launch_impl(ds, c, &q, nullptr, d_counters, hip_stream, ad->h[ad->step & 1].p, "rt_adapt_step",
                             ad->list[ad->cur].p, traced);
  if (rc != RT_OK) return rc;
  ad->samples += ad->px_active * o.step_spp;
  ++ad->step;
  // behind the trace: the tiles' new count, and after an odd step that
  // reached min_spp the rule (at max_spp every tile leaves untested)
  const uint32_t count = static_cast<uint32_t>(ad->step) * static_cast<uint32_t>(o.step_spp);
  const bool even_halves = (ad->step & 1) == 0;
  const bool at_cap = even_halves && count >= static_cast<uint32_t>(o.max_spp);
  const bool decide = even_halves && !at_cap && count >= static_cast<uint32_t>(o.min_spp);
  unsigned* state = ad->state.p + 2 * (ad->gen & 1);
  unsigned* state_next = decide ? ad->state.p + 2 * ((ad->gen + 1) & 1) : nullptr;
  HIP_TRY(enqueue(adapt_eval_kernel, dim3(static_cast<unsigned>((traced + kEvalWaves - 1) / kEvalWaves)),
                  dim3(64 * kEvalWaves), 0, stream, ad->h[0].p, ad->h[1].p, ad->shape.width, ad->rows, ad->gx,
                  ad->list[ad->cur].p, traced, ad->list[ad->cur ^ 1].p, state, state_next, ad->counts.p, count,
                  o.tol_q16, decide ? 1 : 0));
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

extern "C" int64_t rt_adapt_samples(const rt_adapt* ad) { return frame_samples(ad); }

static int adapt_resolve(const rt_adapt* ad, int flags, float* d_f, uint8_t* d_u8, void* hip_stream,
                         const char* who) {
  clear_error();
  if (!ad || (!d_f && !d_u8)) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  if (const int rc = check_resolve_flags(who, flags)) return rc;
  HIP_TRY(hipSetDevice(ad->device));
  const int width = ad->shape.width;
  const unsigned bx = static_cast<unsigned>(std::max(1, std::min((width * 3 / 2 + 255) / 256, 64)));
  // (the rows are the grid's y: rt_adapt_create admits at most 65535)
  HIP_TRY(enqueue(adapt_resolve_kernel, dim3(bx, static_cast<unsigned>(ad->rows)), dim3(256), 0,
                  static_cast<hipStream_t>(hip_stream), ad->h[0].p, ad->h[1].p, ad->counts.p, width, ad->gx,
                  (flags & RT_FLAG_REALM) ? 1 : 0, d_f, d_u8, quantize_table()));
  return RT_OK;
}

extern "C" int rt_adapt_resolve(const rt_adapt* ad, int flags, float* d_out, void* hip_stream) {
  return adapt_resolve(ad, flags, d_out, nullptr, hip_stream, "rt_adapt_resolve");
}

extern "C" int rt_adapt_resolve_u8(const rt_adapt* ad, int flags, uint8_t* d_out, void* hip_stream) {
  return adapt_resolve(ad, flags, nullptr, d_out, hip_stream, "rt_adapt_resolve_u8");
}

extern "C" int rt_adapt_resolve_half(const rt_adapt* ad, int half, int flags, float* d_out, void* hip_stream) {
  clear_error();
  if (!ad || !d_out) return set_error(RT_E_ARG, "rt_adapt_resolve_half: NULL argument");
  if (half != 0 && half != 1) return set_error(RT_E_ARG, "rt_adapt_resolve_half: half is neither 0 nor 1");
  if (const int rc = check_resolve_flags("rt_adapt_resolve_half", flags)) return rc;
  HIP_TRY(hipSetDevice(ad->device));
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((ad->n + 255) / 256, 4096));
  HIP_TRY(enqueue(adapt_half_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                  static_cast<hipStream_t>(hip_stream), ad->h[half].p, ad->counts.p, ad->shape.width, ad->gx, ad->n,
                  (flags & RT_FLAG_REALM) ? 1 : 0, d_out));
  return RT_OK;
}

extern "C" int rt_adapt_counts(const rt_adapt* ad, uint32_t* host_counts, void* hip_stream) {
  clear_error();
  if (!ad || !host_counts) return set_error(RT_E_ARG, "rt_adapt_counts: NULL argument");
  HIP_TRY(hipSetDevice(ad->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_counts, ad->counts.p, ad->n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_adapt_read(const rt_adapt* ad, uint64_t* host_sums0, uint64_t* host_sums1, void* hip_stream) {
  clear_error();
  if (!ad || !host_sums0 || !host_sums1) return set_error(RT_E_ARG, "rt_adapt_read: NULL argument");
  HIP_TRY(hipSetDevice(ad->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_sums0, ad->h[0].p, ad->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(host_sums1, ad->h[1].p, ad->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

// ---- first-hit features: albedo, normal, depth, coverage (rt.h, first_hit.h) ----
// Per pixel six 64-bit sums (albedo rgb, normal xyz, 2^-24 units), a u32 hit
// count and the nearest hit distance as float bits, on the scene's device; the
// samples per pixel they hold on the host side, as rt_accum keeps them.
struct rt_feat : FrameBuf {
  size_t n_px = 0;                   // rows_out x width
  DevBuf<unsigned long long> sums;   // n_px x 6
  DevBuf<unsigned> hits;             // n_px
  DevBuf<unsigned> depth;            // n_px, float bits (+inf: no hit yet)
};

// the feature kernel for a source of bodies (policy::feat_source)
static const void* feat_fn(int src) {
  return src == FEAT_LDS      ? reinterpret_cast<const void*>(&feat_kernel<FEAT_LDS>)
         : src == FEAT_GLOBAL ? reinterpret_cast<const void*>(&feat_kernel<FEAT_GLOBAL>)
                              : reinterpret_cast<const void*>(&feat_kernel<FEAT_SCAN>);
}

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
  if (p->spp == 0) return RT_OK;
  const int rows = rows_out(*p);
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::feat_source(si, g_variant.load(), kDiag);
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
  const int gy = (rows + kTile - 1) / kTile;
  HIP_TRY(enqueue(feat_fn(src), dim3(static_cast<unsigned>(a.tiles_x * gy)), dim3(kFeatThreads), policy::feat_lds(si, src),
                  static_cast<hipStream_t>(hip_stream), a));
  f->samples += p->spp;
  return RT_OK;
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
  const int src = policy::feat_source(si, g_variant.load(), kDiag);
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
  if (stream) {
    hipDevice_t sdev = 0;
    if (hipStreamGetDevice(stream, &sdev) == hipSuccess && static_cast<int>(sdev) != ds->device)
      return set_error(RT_E_ARG, me + ": the stream is on device " + std::to_string(static_cast<int>(sdev)) +
                                     ", the scene on device " + std::to_string(ds->device));
  }
  HIP_TRY(hipSetDevice(ds->device));
  const policy::Scene si = scene_info(*ds);
  const int src = policy::ids_source(si, g_variant.load(), kDiag);
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
  const int src = policy::ids_source(si, g_variant.load(), kDiag);
  if (const int rc = occupancy_report(ids_fn(src), kFeatThreads, policy::feat_lds(si, src), out4)) return rc;
  out4[3] = src;
  return RT_OK;
}

// ---- the denoiser (rt.h, denoise.h) -----------------------------------------
// Its scratch on the device: the two texel arrays the levels ping-pong between
// and the guides the prep packs, for one image size.  mu orders the calls'
// enqueues (the scratch itself is ordered by the caller's stream).
struct rt_denoiser {
  int device = 0, width = 0, rows = 0;
  size_t n_px = 0;
  std::mutex mu;
  DevBuf<DnTexel> tex[2];
  DevBuf<DnGuide> guide;
  DevBuf<float> omc;
};

extern "C" int rt_denoiser_create(int device, int width, int rows, rt_denoiser** out) {
  clear_error();
  if (!out) return set_error(RT_E_ARG, "rt_denoiser_create: NULL argument");
  *out = nullptr;
  // (the level kernel's grid has a block row per kDnBy frame rows)
  if (width <= 0 || rows <= 0 || static_cast<int64_t>(width) * rows > 0x7fffffffll ||
      (rows + kDnBy - 1) / kDnBy > 65535)
    return set_error(RT_E_ARG, "rt_denoiser_create: bad width/rows");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return set_error(RT_E_NODEV, "rt_denoiser_create: device " + std::to_string(device) + " not available");
  HIP_TRY(hipSetDevice(device));
  rt_denoiser* dn = new rt_denoiser;
  dn->device = device;
  dn->width = width;
  dn->rows = rows;
  dn->n_px = static_cast<size_t>(width) * rows;
  hipError_t e = dn->tex[0].alloc(dn->n_px);
  if (e == hipSuccess) e = dn->tex[1].alloc(dn->n_px);
  if (e == hipSuccess) e = dn->guide.alloc(dn->n_px);
  if (e == hipSuccess) e = dn->omc.alloc(dn->n_px);
  if (e != hipSuccess) {
    delete dn;
    return hip_fail(e, "rt_denoiser_create");
  }
  *out = dn;
  return RT_OK;
}

extern "C" int rt_denoiser_free(rt_denoiser* dn) {
  if (!dn) return RT_OK;
  (void)hipSetDevice(dn->device);
  delete dn;
  return RT_OK;
}

static bool dn_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

// rt_denoise / rt_denoise_profile: the checks, then the prep and the levels
// enqueued on the stream.  ev (rt_denoise_profile): 2 + levels events, one
// recorded before the prep and one behind every kernel.
static int denoise_enqueue(const char* who, rt_denoiser* dn, const rt_denoise_opts* o, const float* d_half0,
                           const float* d_half1, const float* d_feat, float* d_out, void* hip_stream,
                           hipEvent_t* ev, int* levels_out) {
  const std::string me(who);
  if (!dn || !d_half0 || !d_half1 || !d_feat || !d_out) return set_error(RT_E_ARG, me + ": NULL argument");
  const rt_denoise_opts opt = o ? *o : dn_default_opts();
  if (const char* why = dn_opts_error(opt)) return set_error(RT_E_ARG, me + ": " + why);
  const size_t cb = dn->n_px * 3 * sizeof(float);
  if (dn_overlap(d_out, cb, d_half0, cb) || dn_overlap(d_out, cb, d_half1, cb) ||
      dn_overlap(d_out, cb, d_feat, dn->n_px * RT_FEAT_CHANNELS * sizeof(float)))
    return set_error(RT_E_ARG, me + ": d_out overlaps an input");
  std::lock_guard<std::mutex> lk(dn->mu);
  HIP_TRY(hipSetDevice(dn->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (stream) {
    hipDevice_t sdev = 0;
    if (hipStreamGetDevice(stream, &sdev) == hipSuccess && static_cast<int>(sdev) != dn->device)
      return set_error(RT_E_ARG, me + ": the stream is on device " + std::to_string(static_cast<int>(sdev)) +
                                     ", the denoiser on device " + std::to_string(dn->device));
  }
  if (levels_out) *levels_out = opt.levels;
  if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
  const size_t pblocks = std::max<size_t>(1, std::min<size_t>((dn->n_px + 255) / 256, 4096));
  HIP_TRY(enqueue(denoise_prep_kernel, dim3(static_cast<unsigned>(pblocks)), dim3(256), 0, stream, d_half0, d_half1,
                  d_feat, dn->n_px, dn->tex[0].p, dn->guide.p, dn->omc.p));
  if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
  const dim3 grid(static_cast<unsigned>((dn->width + kDnBx - 1) / kDnBx),
                  static_cast<unsigned>((dn->rows + kDnBy - 1) / kDnBy)),
      block(kDnBx, kDnBy);
  for (int lv = 0; lv < opt.levels; ++lv) {
    const DnTexel* src = dn->tex[lv & 1].p;
    DnTexel* dst = dn->tex[(lv & 1) ^ 1].p;
    const bool last = lv + 1 == opt.levels;
    if (lv < 2) {   // step 1 and 2: the LDS tile
      const auto fn = lv == 0 ? (last ? denoise_level_lds_kernel<1, true> : denoise_level_lds_kernel<1, false>)
                              : (last ? denoise_level_lds_kernel<2, true> : denoise_level_lds_kernel<2, false>);
      HIP_TRY(enqueue(fn, grid, block, 0, stream, src, dn->guide.p, dn->omc.p, dn->width, dn->rows, opt.normal_pow2,
                      opt.sigma_c, opt.sigma_z, dst, d_feat, d_out));
      if (ev) HIP_TRY(hipEventRecord(ev[2 + lv], stream));
      continue;
    }
    HIP_TRY(enqueue(last ? denoise_level_kernel<true> : denoise_level_kernel<false>, grid, block, 0, stream, src,
                    dn->guide.p, dn->omc.p, dn->width, dn->rows, 1 << lv, opt.normal_pow2, opt.sigma_c, opt.sigma_z,
                    dst, d_feat, d_out));
    if (ev) HIP_TRY(hipEventRecord(ev[2 + lv], stream));
  }
  return RT_OK;
}

extern "C" int rt_denoise(rt_denoiser* dn, const rt_denoise_opts* o, const float* d_half0, const float* d_half1,
                          const float* d_feat, float* d_out, void* hip_stream) {
  clear_error();
  return denoise_enqueue("rt_denoise", dn, o, d_half0, d_half1, d_feat, d_out, hip_stream, nullptr, nullptr);
}

// rt_denoise with an event behind every kernel (diagnostic, tools/denoise_time.py):
// waits, then out_ms = {prep, level 0 .., the whole}.
extern "C" int rt_denoise_profile(rt_denoiser* dn, const rt_denoise_opts* o, const float* d_half0,
                                  const float* d_half1, const float* d_feat, float* d_out, void* hip_stream,
                                  float* out_ms) {
  clear_error();
  if (!out_ms) return set_error(RT_E_ARG, "rt_denoise_profile: NULL argument");
  if (dn) HIP_TRY(hipSetDevice(dn->device));
  hipEvent_t ev[2 + kDnMaxLevels] = {};
  hipError_t e = hipSuccess;
  for (int k = 0; dn && k < 2 + kDnMaxLevels && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
  int levels = 0;
  int rc = e == hipSuccess ? denoise_enqueue("rt_denoise_profile", dn, o, d_half0, d_half1, d_feat, d_out, hip_stream,
                                             ev, &levels)
                           : hip_fail(e, "rt_denoise_profile");
  if (rc == RT_OK) {
    e = hipEventSynchronize(ev[1 + levels]);
    for (int k = 0; k <= levels && e == hipSuccess; ++k) e = hipEventElapsedTime(&out_ms[k], ev[k], ev[k + 1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&out_ms[levels + 1], ev[0], ev[1 + levels]);
    if (e != hipSuccess) rc = hip_fail(e, "rt_denoise_profile");
  }
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  return rc;
}

// ---- temporal accumulation (rt.h, temporal.h) --------------------------------
// The history on the device: two sets of three packed arrays -- a step gathers
// from set `cur` and writes set cur ^ 1 -- and, on the host, the camera that
// wrote set `cur`.  mu orders the calls' enqueues (the sets themselves are
// ordered by the caller's stream).
struct rt_temporal {
  int device = 0, width = 0, rows = 0, row0 = 0;
  size_t n_px = 0;
  mutable std::mutex mu;
  DevBuf<TpWord> a0[2], a1[2];
  DevBuf<DnGuide> guide[2];
  DevBuf<TpWord> box;   // the clamp's scratch: n_px lo words, then n_px hi words (the first clamp step allocates it)
  int cur = 0;
  bool have_prev = false;
  rt_camera prev{};
  int64_t frames = 0;
};

extern "C" int rt_temporal_create(int device, int width, int rows, int row0, rt_temporal** out) {
  clear_error();
  if (!out) return set_error(RT_E_ARG, "rt_temporal_create: NULL argument");
  *out = nullptr;
  if (const char* why = tp_shape_error(width, rows, row0))
    return set_error(RT_E_ARG, std::string("rt_temporal_create: ") + why);
  // (the kernel's grid has a block row per kDnBy image rows)
  if ((rows + kDnBy - 1) / kDnBy > 65535) return set_error(RT_E_ARG, "rt_temporal_create: bad width/rows");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return set_error(RT_E_NODEV, "rt_temporal_create: device " + std::to_string(device) + " not available");
  HIP_TRY(hipSetDevice(device));
  rt_temporal* t = new rt_temporal;
  t->device = device;
  t->width = width;
  t->rows = rows;
  t->row0 = row0;
  t->n_px = static_cast<size_t>(width) * rows;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = t->a0[k].alloc(t->n_px);
    if (e == hipSuccess) e = t->a1[k].alloc(t->n_px);
    if (e == hipSuccess) e = t->guide[k].alloc(t->n_px);
  }
  // the set a first rt_temporal_read shows: L = 0 everywhere
  if (e == hipSuccess) e = fill_zero(t->a0[0], t->n_px, nullptr);
  if (e == hipSuccess) e = fill_zero(t->a1[0], t->n_px, nullptr);
  if (e == hipSuccess) e = fill_zero(t->guide[0], t->n_px, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    delete t;
    return hip_fail(e, "rt_temporal_create");
  }
  *out = t;
  return RT_OK;
}

extern "C" int rt_temporal_free(rt_temporal* t) {
  if (!t) return RT_OK;
  (void)hipSetDevice(t->device);
  delete t;
  return RT_OK;
}

// nullptr's device, or whether `stream` belongs to t's device
static int tp_stream_check(const std::string& me, const rt_temporal* t, hipStream_t stream) {
  if (stream) {
    hipDevice_t sdev = 0;
    if (hipStreamGetDevice(stream, &sdev) == hipSuccess && static_cast<int>(sdev) != t->device)
      return set_error(RT_E_ARG, me + ": the stream is on device " + std::to_string(static_cast<int>(sdev)) +
                                     ", the history on device " + std::to_string(t->device));
  }
  return RT_OK;
}

extern "C" int rt_temporal_reset(rt_temporal* t, void* hip_stream) {
  clear_error();
  if (!t) return set_error(RT_E_ARG, "rt_temporal_reset: NULL argument");
  std::lock_guard<std::mutex> lk(t->mu);
  HIP_TRY(hipSetDevice(t->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = tp_stream_check("rt_temporal_reset", t, stream)) return rc;
  HIP_TRY(fill_zero(t->a0[t->cur], t->n_px, stream));
  HIP_TRY(fill_zero(t->a1[t->cur], t->n_px, stream));
  HIP_TRY(fill_zero(t->guide[t->cur], t->n_px, stream));
  t->have_prev = false;
  t->frames = 0;
  return RT_OK;
}

extern "C" int64_t rt_temporal_frames(const rt_temporal* t) {
  if (!t) return -1;
  std::lock_guard<std::mutex> lk(t->mu);
  return t->frames;
}

// rt_temporal_step (MOTION == false: d_ids, d_motion and n_bodies are not
// looked at), rt_temporal_step_motion and rt_temporal_step_clamp (CLAMP; k is
// looked at with it only): the checks, the set-up, one kernel -- with CLAMP
// and history, the box kernel before it.  WEIGHT (rt_temporal_step_budget):
// d_mult is the band's gy x gx multipliers, and CLAMP then says whether the
// box is built (k is checked either way); without it d_mult is not looked at.
template <bool MOTION, bool CLAMP, bool WEIGHT = false>
static int temporal_step(const std::string& me, rt_temporal* t, const rt_temporal_opts* o,
                         const rt_temporal_clamp_opts* k, const rt_camera* cam, const float* d_half0,
                         const float* d_half1, const float* d_feat, const int32_t* d_ids, const float* d_motion,
                         int n_bodies, float* d_out0, float* d_out1, void* hip_stream,
                         const uint32_t* d_mult = nullptr) {
  clear_error();
  if (!t || !cam || !d_half0 || !d_half1 || !d_feat || !d_out0 || !d_out1 || (WEIGHT && !d_mult))
    return set_error(RT_E_ARG, me + ": NULL argument");
  if (MOTION) {
    if (const char* why = tp_motion_error(d_ids, d_motion, n_bodies)) return set_error(RT_E_ARG, me + ": " + why);
    if (reinterpret_cast<uintptr_t>(d_motion) % 16 != 0) return set_error(RT_E_ARG, me + ": d_motion is not 16-byte aligned");
  }
  const rt_temporal_opts opt = o ? *o : tp_default_opts();
  if (const char* why = tp_opts_error(opt)) return set_error(RT_E_ARG, me + ": " + why);
  const rt_temporal_clamp_opts kopt = (CLAMP || WEIGHT) && k ? *k : tp_default_clamp_opts();
  if (CLAMP || WEIGHT)
    if (const char* why = tp_clamp_opts_error(kopt)) return set_error(RT_E_ARG, me + ": " + why);
  const size_t cb = t->n_px * 3 * sizeof(float), fb = t->n_px * RT_FEAT_CHANNELS * sizeof(float);
  const size_t wb = !WEIGHT ? 0
                            : static_cast<size_t>((t->width + kTpTile - 1) / kTpTile) * ((t->rows + kTpTile - 1) / kTpTile) *
                                  sizeof(uint32_t);
  const size_t ib = MOTION ? t->n_px * sizeof(int32_t) : 0, mb = MOTION ? static_cast<size_t>(n_bodies) * 4 * sizeof(float) : 0;
  for (const float* d_out : {d_out0, d_out1})
    if (tp_overlap(d_out, cb, d_half0, cb) || tp_overlap(d_out, cb, d_half1, cb) || tp_overlap(d_out, cb, d_feat, fb) ||
        tp_overlap(d_out, cb, d_ids, ib) || tp_overlap(d_out, cb, d_motion, mb) || tp_overlap(d_out, cb, d_mult, wb))
      return set_error(RT_E_ARG, me + ": an output overlaps an input");
  if (tp_overlap(d_out0, cb, d_out1, cb)) return set_error(RT_E_ARG, me + ": the outputs overlap");
  std::lock_guard<std::mutex> lk(t->mu);
  TpFrame f = tp_frame(opt, *cam, t->width, t->rows, t->row0);
  if (t->have_prev) {
    if (!tp_setup(*cam, t->prev, f.R, f.dc))
      return set_error(RT_E_ARG, me + ": the previous camera is degenerate (det is 0 or not finite)");
    f.have_prev = 1;
  }
  HIP_TRY(hipSetDevice(t->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = tp_stream_check(me, t, stream)) return rc;
  if (CLAMP && !t->box) HIP_TRY(t->box.alloc(2 * t->n_px));
  const int src = t->cur, dst = t->cur ^ 1;
  const dim3 grid(static_cast<unsigned>((t->width + kDnBx - 1) / kDnBx),
                  static_cast<unsigned>((t->rows + kDnBy - 1) / kDnBy)),
      block(kDnBx, kDnBy);
  if (CLAMP) {
    TpWord *box_lo = t->box.p, *box_hi = t->box.p + t->n_px;
    const auto box_fn = kopt.radius == 1   ? temporal_box_kernel<1>
                        : kopt.radius == 2 ? temporal_box_kernel<2>
                                           : temporal_box_kernel<3>;
    if (f.have_prev)   // (the first step after create or reset has no history to clamp)
      HIP_TRY(enqueue(box_fn, grid, block, 0, stream, d_half0, d_half1, d_feat, t->width, t->rows,
                      f.sigma_z, f.normal_min, kopt.gamma, box_lo, box_hi));
    if (WEIGHT)
      HIP_TRY(enqueue(temporal_step_budget_kernel<MOTION, true>, grid, block, 0, stream, f, d_half0, d_half1, d_feat,
                      d_ids, d_motion, n_bodies, d_mult, static_cast<const TpWord*>(box_lo),
                      static_cast<const TpWord*>(box_hi), t->a0[src].p, t->a1[src].p, t->guide[src].p, t->a0[dst].p,
                      t->a1[dst].p, t->guide[dst].p, d_out0, d_out1));
    else
      HIP_TRY(enqueue(temporal_step_clamp_kernel<MOTION>, grid, block, 0, stream, f, d_half0, d_half1, d_feat, d_ids,
                      d_motion, n_bodies, static_cast<const TpWord*>(box_lo), static_cast<const TpWord*>(box_hi),
                      t->a0[src].p, t->a1[src].p, t->guide[src].p, t->a0[dst].p, t->a1[dst].p, t->guide[dst].p, d_out0,
                      d_out1));
  } else if (WEIGHT)
    HIP_TRY(enqueue(temporal_step_budget_kernel<MOTION, false>, grid, block, 0, stream, f, d_half0, d_half1, d_feat,
                    d_ids, d_motion, n_bodies, d_mult, static_cast<const TpWord*>(nullptr),
                    static_cast<const TpWord*>(nullptr), t->a0[src].p, t->a1[src].p, t->guide[src].p, t->a0[dst].p,
                    t->a1[dst].p, t->guide[dst].p, d_out0, d_out1));
  else if (MOTION)
    HIP_TRY(enqueue(temporal_step_motion_kernel, grid, block, 0, stream, f, d_half0, d_half1, d_feat, d_ids, d_motion,
                    n_bodies, t->a0[src].p, t->a1[src].p, t->guide[src].p, t->a0[dst].p, t->a1[dst].p, t->guide[dst].p,
                    d_out0, d_out1));
  else
    HIP_TRY(enqueue(temporal_step_kernel, grid, block, 0, stream, f, d_half0, d_half1, d_feat, t->a0[src].p,
                    t->a1[src].p, t->guide[src].p, t->a0[dst].p, t->a1[dst].p, t->guide[dst].p, d_out0, d_out1));
  t->cur = dst;
  t->prev = *cam;
  t->have_prev = true;
  t->frames += 1;
  return RT_OK;
}

extern "C" int rt_temporal_step(rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam, const float* d_half0,
                                const float* d_half1, const float* d_feat, float* d_out0, float* d_out1,
                                void* hip_stream) {
  return temporal_step<false, false>("rt_temporal_step", t, o, nullptr, cam, d_half0, d_half1, d_feat, nullptr, nullptr,
                                     0, d_out0, d_out1, hip_stream);
}

extern "C" int rt_temporal_step_motion(rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam,
                                       const float* d_half0, const float* d_half1, const float* d_feat,
                                       const int32_t* d_ids, const float* d_motion, int n_bodies, float* d_out0,
                                       float* d_out1, void* hip_stream) {
  return temporal_step<true, false>("rt_temporal_step_motion", t, o, nullptr, cam, d_half0, d_half1, d_feat, d_ids,
                                    d_motion, n_bodies, d_out0, d_out1, hip_stream);
}

// raytracing.clj:141-155's frames with the fetched history held to the current
// frame's colour box (rt.h); d_ids == NULL: rt_temporal_step's reprojection
extern "C" int rt_temporal_step_clamp(rt_temporal* t, const rt_temporal_opts* o, const rt_temporal_clamp_opts* k,
                                      const rt_camera* cam, const float* d_half0, const float* d_half1,
                                      const float* d_feat, const int32_t* d_ids, const float* d_motion, int n_bodies,
                                      float* d_out0, float* d_out1, void* hip_stream) {
  const std::string me("rt_temporal_step_clamp");
  if (!d_ids)
    return temporal_step<false, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, nullptr, nullptr, 0, d_out0, d_out1,
                                      hip_stream);
  return temporal_step<true, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, d_ids, d_motion, n_bodies, d_out0,
                                   d_out1, hip_stream);
}

extern "C" int rt_temporal_read(const rt_temporal* t, float* host_a0, float* host_a1, float* host_guide,
                                float* host_len, void* hip_stream) {
  clear_error();
  if (!t) return set_error(RT_E_ARG, "rt_temporal_read: NULL argument");
  std::lock_guard<std::mutex> lk(t->mu);
  HIP_TRY(hipSetDevice(t->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = tp_stream_check("rt_temporal_read", t, stream)) return rc;
  std::vector<TpWord> w0, w1;
  if (host_a0 || host_len) {
    w0.resize(t->n_px);
    HIP_TRY(hipMemcpyAsync(w0.data(), t->a0[t->cur].p, t->n_px * sizeof(TpWord), hipMemcpyDeviceToHost, stream));
  }
  if (host_a1) {
    w1.resize(t->n_px);
    HIP_TRY(hipMemcpyAsync(w1.data(), t->a1[t->cur].p, t->n_px * sizeof(TpWord), hipMemcpyDeviceToHost, stream));
  }
  if (host_guide)
    HIP_TRY(hipMemcpyAsync(host_guide, t->guide[t->cur].p, t->n_px * sizeof(DnGuide), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (size_t i = 0; i < t->n_px; ++i) {
    if (host_a0) {
      host_a0[3 * i] = w0[i].r;
      host_a0[3 * i + 1] = w0[i].g;
      host_a0[3 * i + 2] = w0[i].b;
    }
    if (host_len) host_len[i] = w0[i].l;
    if (host_a1) {
      host_a1[3 * i] = w1[i].r;
      host_a1[3 * i + 1] = w1[i].g;
      host_a1[3 * i + 2] = w1[i].b;
    }
  }
  return RT_OK;
}

static int stream_on_device(const std::string& me, hipStream_t stream, int device);   // (below)

// ---- the sample budget (rt.h, budget.h, temporal.h) ----------
// rt_temporal_step_budget: rt_temporal_step_clamp's step with the tiles'
// weights; gamma = +inf clamps nothing (rt.h), so no box is built then.
extern "C" int rt_temporal_step_budget(rt_temporal* t, const rt_temporal_opts* o, const rt_temporal_clamp_opts* k,
                                       const rt_camera* cam, const float* d_half0, const float* d_half1,
                                       const float* d_feat, const int32_t* d_ids, const float* d_motion, int n_bodies,
                                       const uint32_t* d_mult, float* d_out0, float* d_out1, void* hip_stream) {
  const std::string me("rt_temporal_step_budget");
  const bool box = !(k && k->gamma == INFINITY);
  if (!d_ids)
    return box ? temporal_step<false, true, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, nullptr, nullptr, 0, d_out0,
                                                  d_out1, hip_stream, d_mult)
               : temporal_step<false, false, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, nullptr, nullptr, 0,
                                                   d_out0, d_out1, hip_stream, d_mult);
  return box ? temporal_step<true, true, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, d_ids, d_motion, n_bodies,
                                               d_out0, d_out1, hip_stream, d_mult)
             : temporal_step<true, false, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, d_ids, d_motion, n_bodies,
                                                d_out0, d_out1, hip_stream, d_mult);
}

// rt_temporal_probe: the step's checks and set-up, one kernel, no state touched
extern "C" int rt_temporal_probe(const rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam,
                                 const float* d_feat, const int32_t* d_ids, const float* d_motion, int n_bodies,
                                 float* d_len, void* hip_stream) {
  clear_error();
  const std::string me("rt_temporal_probe");
  if (!t || !cam || !d_feat || !d_len) return set_error(RT_E_ARG, me + ": NULL argument");
  if (d_ids) {
    if (const char* why = tp_motion_error(d_ids, d_motion, n_bodies)) return set_error(RT_E_ARG, me + ": " + why);
    if (reinterpret_cast<uintptr_t>(d_motion) % 16 != 0) return set_error(RT_E_ARG, me + ": d_motion is not 16-byte aligned");
  }
  const rt_temporal_opts opt = o ? *o : tp_default_opts();
  if (const char* why = tp_opts_error(opt)) return set_error(RT_E_ARG, me + ": " + why);
  const size_t lb = t->n_px * sizeof(float), fb = t->n_px * RT_FEAT_CHANNELS * sizeof(float);
  const size_t ib = d_ids ? t->n_px * sizeof(int32_t) : 0, mb = d_ids ? static_cast<size_t>(n_bodies) * 4 * sizeof(float) : 0;
  if (tp_overlap(d_len, lb, d_feat, fb) || tp_overlap(d_len, lb, d_ids, ib) || tp_overlap(d_len, lb, d_motion, mb))
    return set_error(RT_E_ARG, me + ": the output overlaps an input");
  std::lock_guard<std::mutex> lk(t->mu);
  TpFrame f = tp_frame(opt, *cam, t->width, t->rows, t->row0);
  if (t->have_prev) {
    if (!tp_setup(*cam, t->prev, f.R, f.dc))
      return set_error(RT_E_ARG, me + ": the previous camera is degenerate (det is 0 or not finite)");
    f.have_prev = 1;
  }
  HIP_TRY(hipSetDevice(t->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = tp_stream_check(me, t, stream)) return rc;
  const dim3 grid(static_cast<unsigned>((t->width + kDnBx - 1) / kDnBx),
                  static_cast<unsigned>((t->rows + kDnBy - 1) / kDnBy)),
      block(kDnBx, kDnBy);
  const TpWord* a0 = t->a0[t->cur].p;
  const DnGuide* g = t->guide[t->cur].p;
  if (d_ids)
    HIP_TRY(enqueue(temporal_probe_kernel<true>, grid, block, 0, stream, f, d_feat, d_ids, d_motion, n_bodies, a0, g,
                    d_len));
  else
    HIP_TRY(enqueue(temporal_probe_kernel<false>, grid, block, 0, stream, f, d_feat, static_cast<const int32_t*>(nullptr),
                    static_cast<const float*>(nullptr), 0, a0, g, d_len));
  return RT_OK;
}

// The budgeted frame: h[0], h[1] the sums of the even and the odd sample
// blocks in the accumulator's layout; mult and counts per 8 x 8 tile of the
// output rows; list: every tile, by descending mult; state: the plan kernels'
// scratch; back: what the list kernel leaves for the host (n_j, px_j), copied
// to `pinned` behind it -- rt_budget_trace waits for `ev` and takes the grids
// of its launches from there.
struct rt_budget : FrameBuf {
  rt_budget_opts opts{};
  int rows = 0, gx = 0, gy = 0, n_tiles = 0;
  size_t n = 0;   // sums per half: rows x width x 3
  DevBuf<unsigned long long> h[2];
  DevBuf<uint32_t> mult, counts;
  DevBuf<int> list;
  DevBuf<unsigned> state, back;   // device u32[kBdState], u32[kBdBack]
  unsigned* pinned = nullptr;     // host u32[kBdBack]
  hipEvent_t ev = nullptr;
  bool pending = false;   // a plan's read-back is in flight
  bool planned = false;   // a plan no trace has used yet
  bool have = false;      // nj, px hold a plan's numbers
  unsigned nj[kBdMaxMult] = {}, px[kBdMaxMult] = {};
  ~rt_budget() {
    if (pinned) (void)hipHostFree(pinned);
    if (ev) (void)hipEventDestroy(ev);
  }
};

extern "C" int rt_budget_create(const rt_dscene* ds, const rt_params* shape, const rt_budget_opts* opts,
                                rt_budget** out) {
  clear_error();
  if (out) *out = nullptr;
  if (!ds || !shape || !opts || !out) return set_error(RT_E_ARG, "rt_budget_create: NULL argument");
  if (const char* why = bd_opts_error(*opts)) return set_error(RT_E_ARG, std::string("rt_budget_create: ") + why);
  if (shape->tile_step != 0) return set_error(RT_E_ARG, "rt_budget_create: tile_step must be 0 (a contiguous band)");
  int rows = 0;
  if (const int rc = frame_rows("rt_budget_create", *shape, &rows)) return rc;
  const int64_t tiles = static_cast<int64_t>((shape->width + kTile - 1) / kTile) * ((rows + kTile - 1) / kTile);
  // (the resolve's grid has a block row per frame row; the pixel counts are u32)
  if (rows > 65535 || tiles > INT_MAX / policy::kSplitMax || static_cast<int64_t>(rows) * shape->width > 0xffffffffll)
    return set_error(RT_E_ARG, "rt_budget_create: frame too large (more than 65535 rows)");
  rt_budget* bd = nullptr;
  if (const int rc = frame_new(*ds, *shape, &bd)) return rc;
  bd->opts = *opts;
  bd->rows = rows;
  bd->gx = (shape->width + kTile - 1) / kTile;
  bd->gy = (rows + kTile - 1) / kTile;
  bd->n_tiles = static_cast<int>(tiles);
  bd->n = static_cast<size_t>(rows) * shape->width * 3;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = bd->h[k].alloc(bd->n);
    if (e == hipSuccess) e = fill_zero(bd->h[k], bd->n, nullptr);
  }
  if (e == hipSuccess) e = bd->mult.alloc(bd->n_tiles);
  if (e == hipSuccess) e = bd->counts.alloc(bd->n_tiles);
  if (e == hipSuccess) e = bd->list.alloc(bd->n_tiles);
  if (e == hipSuccess) e = bd->state.alloc(kBdState);
  if (e == hipSuccess) e = bd->back.alloc(kBdBack);
  if (e == hipSuccess) e = fill_zero(bd->mult, bd->n_tiles, nullptr);
  if (e == hipSuccess) e = fill_zero(bd->counts, bd->n_tiles, nullptr);
  if (e == hipSuccess) e = fill_zero(bd->list, bd->n_tiles, nullptr);   // (every entry a tile of the frame, always)
  if (e == hipSuccess) e = hipHostMalloc(&bd->pinned, kBdBack * sizeof(unsigned));
  if (e == hipSuccess) e = hipEventCreateWithFlags(&bd->ev, hipEventDisableTiming);
  return frame_created("rt_budget_create", bd, e, out);
}

extern "C" int rt_budget_free(rt_budget* bd) {
  if (bd && bd->pending) (void)hipEventSynchronize(bd->ev);   // (the copy into `pinned`)
  return frame_free(bd);
}

// the read-back in flight, if any: wait for it and take its numbers (the caller holds bd->mu)
static int budget_settle(rt_budget* bd) {
  if (!bd->pending) return RT_OK;
  HIP_TRY(hipEventSynchronize(bd->ev));
  bd->pending = false;
  for (int j = 0; j < kBdMaxMult; ++j) {
    bd->nj[j] = bd->pinned[j];
    bd->px[j] = bd->pinned[kBdMaxMult + j];
  }
  bd->have = true;
  return RT_OK;
}

// rt_budget_plan (d_len) and rt_budget_plan_mult (d_mult): the zeroing, the
// plan or the clamp kernel, the list kernel, the read-back
static int budget_plan(const char* who, rt_budget* bd, const float* d_len, const uint32_t* d_mult, void* hip_stream) {
  clear_error();
  if (!bd || (!d_len && !d_mult)) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  std::lock_guard<std::mutex> lk(bd->mu);
  HIP_TRY(hipSetDevice(bd->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device(who, stream, bd->device)) return rc;
  if (bd->pending) HIP_TRY(hipEventSynchronize(bd->ev));   // (`pinned` is about to be written again)
  bd->pending = bd->planned = bd->have = false;
  for (int k = 0; k < 2; ++k) HIP_TRY(fill_zero(bd->h[k], bd->n, stream));
  HIP_TRY(fill_zero(bd->state, kBdState, stream));
  const rt_budget_opts& o = bd->opts;
  const int width = bd->shape.width, nt = bd->n_tiles;
  if (d_len)
    HIP_TRY(enqueue(budget_plan_kernel, dim3(static_cast<unsigned>((nt + kBdPlanWaves - 1) / kBdPlanWaves)),
                    dim3(64 * kBdPlanWaves), 0, stream, d_len, width, bd->rows, bd->gx, nt, o.target, o.max_mult,
                    o.quantile_64, bd->mult.p, bd->state.p));
  else
    HIP_TRY(enqueue(budget_clamp_kernel, dim3(static_cast<unsigned>((nt + 255) / 256)), dim3(256), 0, stream, d_mult,
                    width, bd->rows, bd->gx, nt, o.max_mult, bd->mult.p, bd->state.p));
  HIP_TRY(enqueue(budget_list_kernel, dim3(static_cast<unsigned>((nt + 255) / 256)), dim3(256), 0, stream,
                  static_cast<const uint32_t*>(bd->mult.p), nt, o.half_spp, bd->state.p, bd->list.p, bd->counts.p,
                  bd->back.p));
  HIP_TRY(hipMemcpyAsync(bd->pinned, bd->back.p, kBdBack * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipEventRecord(bd->ev, stream));
  bd->pending = bd->planned = true;
  return RT_OK;
}

extern "C" int rt_budget_plan(rt_budget* bd, const float* d_len, void* hip_stream) {
  if (!d_len) {
    clear_error();
    return set_error(RT_E_ARG, "rt_budget_plan: NULL argument");
  }
  return budget_plan("rt_budget_plan", bd, d_len, nullptr, hip_stream);
}

extern "C" int rt_budget_plan_mult(rt_budget* bd, const uint32_t* d_mult, void* hip_stream) {
  return budget_plan("rt_budget_plan_mult", bd, nullptr, d_mult, hip_stream);
}

extern "C" int rt_budget_trace(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_budget* bd,
                               uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!ds || !c || !p || !bd) return set_error(RT_E_ARG, "rt_budget_trace: NULL argument");
  if (const int rc = check_match("rt_budget_trace", "the budgeted frame", *bd, *ds, *p)) return rc;
  std::lock_guard<std::mutex> lk(bd->mu);
  if (!bd->planned) return set_error(RT_E_ARG, "rt_budget_trace: no fresh plan (rt_budget_plan comes first)");
  const rt_budget_opts& o = bd->opts;
  if (p->sample_begin < 0 || static_cast<int64_t>(p->sample_begin) + 2ll * o.max_mult * o.half_spp > INT_MAX)
    return set_error(RT_E_ARG, "rt_budget_trace: sample_begin + 2 * max_mult * half_spp passes 2^31 - 1");
  HIP_TRY(hipSetDevice(bd->device));
  if (const int rc = budget_settle(bd)) return rc;
  int launches = 0;
  for (int j = 0; j < o.max_mult; ++j) {
    const int n_j = static_cast<int>(std::min<unsigned>(bd->nj[j], static_cast<unsigned>(bd->n_tiles)));
    if (n_j <= 0) break;   // (the n_j do not grow)
    for (int h = 0; h < 2; ++h) {
      rt_params q = *p;
      q.spp = o.half_spp;
      q.sample_begin = p->sample_begin + (2 * j + h) * o.half_spp;
      // (a refusal comes from the first launch, before anything is enqueued: the variant's tiles)
      if (const int rc = launch_impl(ds, c, &q, nullptr, d_counters, hip_stream, bd->h[h].p, "rt_budget_trace",
                                     bd->list.p, n_j))
        return rc;
      ++launches;
    }
  }
  bd->planned = false;
  return launches;
}

extern "C" int rt_budget_resolve(const rt_budget* bd, int flags, float* d_out, void* hip_stream) {
  clear_error();
  if (!bd || !d_out) return set_error(RT_E_ARG, "rt_budget_resolve: NULL argument");
  if (const int rc = check_resolve_flags("rt_budget_resolve", flags)) return rc;
  HIP_TRY(hipSetDevice(bd->device));
  const int width = bd->shape.width;
  const unsigned bx = static_cast<unsigned>(std::max(1, std::min((width * 3 / 2 + 255) / 256, 64)));
  // (the rows are the grid's y: rt_budget_create admits at most 65535)
  HIP_TRY(enqueue(adapt_resolve_kernel, dim3(bx, static_cast<unsigned>(bd->rows)), dim3(256), 0,
                  static_cast<hipStream_t>(hip_stream), bd->h[0].p, bd->h[1].p, bd->counts.p, width, bd->gx,
                  (flags & RT_FLAG_REALM) ? 1 : 0, d_out, static_cast<uint8_t*>(nullptr), quantize_table()));
  return RT_OK;
}

extern "C" int rt_budget_resolve_half(const rt_budget* bd, int half, int flags, float* d_out, void* hip_stream) {
  clear_error();
  if (!bd || !d_out) return set_error(RT_E_ARG, "rt_budget_resolve_half: NULL argument");
  if (half != 0 && half != 1) return set_error(RT_E_ARG, "rt_budget_resolve_half: half is neither 0 nor 1");
  if (const int rc = check_resolve_flags("rt_budget_resolve_half", flags)) return rc;
  HIP_TRY(hipSetDevice(bd->device));
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((bd->n + 255) / 256, 4096));
  HIP_TRY(enqueue(adapt_half_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                  static_cast<hipStream_t>(hip_stream), bd->h[half].p, bd->counts.p, bd->shape.width, bd->gx, bd->n,
                  (flags & RT_FLAG_REALM) ? 1 : 0, d_out));
  return RT_OK;
}

extern "C" int rt_budget_read(const rt_budget* bd, uint64_t* host_sums0, uint64_t* host_sums1, void* hip_stream) {
  clear_error();
  if (!bd || !host_sums0 || !host_sums1) return set_error(RT_E_ARG, "rt_budget_read: NULL argument");
  HIP_TRY(hipSetDevice(bd->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_sums0, bd->h[0].p, bd->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(host_sums1, bd->h[1].p, bd->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_budget_mult_read(const rt_budget* bd, uint32_t* host_mult, void* hip_stream) {
  clear_error();
  if (!bd || !host_mult) return set_error(RT_E_ARG, "rt_budget_mult_read: NULL argument");
  HIP_TRY(hipSetDevice(bd->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_mult, bd->mult.p, bd->n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_budget_device_mult(const rt_budget* bd, const uint32_t** d_mult) {
  clear_error();
  if (!bd || !d_mult) return set_error(RT_E_ARG, "rt_budget_device_mult: NULL argument");
  *d_mult = bd->mult.p;
  return RT_OK;
}

extern "C" int64_t rt_budget_samples(rt_budget* bd) {
  if (!bd) return 0;
  std::lock_guard<std::mutex> lk(bd->mu);
  (void)hipSetDevice(bd->device);
  if (budget_settle(bd) != RT_OK || !bd->have) return 0;
  int64_t px = 0;   // sum over j of the pixels of the tiles with mult > j = sum over tiles of npx * mult
  for (int j = 0; j < bd->opts.max_mult; ++j) px += bd->px[j];
  return px * 2 * bd->opts.half_spp;
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

// ---- rt_scene_update (rt.h, bvh_refit.h) -------------------------------------
// (The last section of the file, and refit_kernel a template, on purpose: a
// template's code is emitted where it is first instantiated, so the refit
// kernel follows every other kernel in the code object and none of them moves.)
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

static int stream_on_device(const std::string& me, hipStream_t stream, int device) {
  if (!stream) return RT_OK;
  hipDevice_t sdev = 0;
  if (hipStreamGetDevice(stream, &sdev) == hipSuccess && static_cast<int>(sdev) != device)
    return set_error(RT_E_ARG, me + ": the stream is on device " + std::to_string(static_cast<int>(sdev)) +
                                   ", the scene on device " + std::to_string(device));
  return RT_OK;
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
  if (const int rc = stream_on_device(me, stream, ds->device)) return rc;
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
  if (const int rc = stream_on_device(me, stream, ds->device)) return rc;
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
