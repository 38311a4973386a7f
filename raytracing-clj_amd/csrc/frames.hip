// frames.hip — the frames whose integer sums outlive the launches: the
// accumulator (rt_accum), the adaptive sampler (rt_adapt) and the sample budget
// (rt_budget; budget.h's plan kernels), with their resolve, add and evaluation
// kernels.  Their passes are the trace unit's launch_impl (dscene.h).
// DESIGN.md §3.5, §3.6, §3.13.
#include "trace_kernel.h"
#define RT_BUDGET_KERNEL
#include "budget.h"
#include "dscene.h"

namespace rtclj {

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
}  // namespace rtclj

using namespace rtclj;

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

// ---- two half accumulators over 8 x 8 tiles: what rt_adapt and rt_budget share ----
// h[0], h[1]: the sums of the even and the odd steps (sample blocks), in the
// accumulator's layout; counts: samples per pixel of each 8 x 8 tile of the
// output rows.  What the entry's kernels leave for the host is copied to
// `pinned` behind them; the call that needs it waits for `ev`.
struct HalfFrames : FrameBuf {
  int rows = 0, gx = 0, gy = 0, n_tiles = 0;
  size_t n = 0;   // sums per half: rows x width x 3
  DevBuf<unsigned long long> h[2];
  DevBuf<uint32_t> counts;
  unsigned* pinned = nullptr;   // host u32[2] (rt_adapt), u32[kBdBack] (rt_budget)
  hipEvent_t ev = nullptr;
  bool pending = false;   // a read-back is in flight
  ~HalfFrames() {
    if (pinned) (void)hipHostFree(pinned);
    if (ev) (void)hipEventDestroy(ev);
  }
};

// a create's new frame (rt_adapt, rt_budget) for `shape` on ds's device: its
// rows and tile grid set, nothing allocated yet
template <class B>
static int halves_new(const char* who, const rt_dscene& ds, const rt_params& shape, B** out) {
  int rows = 0;
  if (const int rc = frame_rows(who, shape, &rows)) return rc;
  const int64_t tiles = static_cast<int64_t>((shape.width + kTile - 1) / kTile) * ((rows + kTile - 1) / kTile);
  // (the resolve's grid has a block row per frame row; the pixel counts are u32)
  if (rows > 65535 || tiles > INT_MAX / policy::kSplitMax || static_cast<int64_t>(rows) * shape.width > 0xffffffffll)
    return set_error(RT_E_ARG, std::string(who) + ": frame too large (more than 65535 rows)");
  if (const int rc = frame_new(ds, shape, out)) return rc;
  B* b = *out;
  b->rows = rows;
  b->gx = (shape.width + kTile - 1) / kTile;
  b->gy = (rows + kTile - 1) / kTile;
  b->n_tiles = static_cast<int>(tiles);
  b->n = static_cast<size_t>(rows) * shape.width * 3;
  return RT_OK;
}

// h0 + h1 as a frame of floats and / or bytes
static int halves_resolve(const char* who, const HalfFrames* b, int flags, float* d_f, uint8_t* d_u8, void* hip_stream) {
  clear_error();
  if (!b || (!d_f && !d_u8)) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  if (const int rc = check_resolve_flags(who, flags)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const int width = b->shape.width;
  const unsigned bx = static_cast<unsigned>(std::max(1, std::min((width * 3 / 2 + 255) / 256, 64)));
  // (the rows are the grid's y: the creates admit at most 65535)
  HIP_TRY(enqueue(adapt_resolve_kernel, dim3(bx, static_cast<unsigned>(b->rows)), dim3(256), 0,
                  static_cast<hipStream_t>(hip_stream), b->h[0].p, b->h[1].p, b->counts.p, width, b->gx,
                  (flags & RT_FLAG_REALM) ? 1 : 0, d_f, d_u8, quantize_table()));
  return RT_OK;
}

static int halves_resolve_half(const char* who, const HalfFrames* b, int half, int flags, float* d_out, void* hip_stream) {
  clear_error();
  if (!b || !d_out) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  if (half != 0 && half != 1) return set_error(RT_E_ARG, std::string(who) + ": half is neither 0 nor 1");
  if (const int rc = check_resolve_flags(who, flags)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((b->n + 255) / 256, 4096));
  HIP_TRY(enqueue(adapt_half_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                  static_cast<hipStream_t>(hip_stream), b->h[half].p, b->counts.p, b->shape.width, b->gx, b->n,
                  (flags & RT_FLAG_REALM) ? 1 : 0, d_out));
  return RT_OK;
}

static int halves_read(const char* who, const HalfFrames* b, uint64_t* host_sums0, uint64_t* host_sums1, void* hip_stream) {
  clear_error();
  if (!b || !host_sums0 || !host_sums1) return set_error(RT_E_ARG, std::string(who) + ": NULL argument");
  HIP_TRY(hipSetDevice(b->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_sums0, b->h[0].p, b->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(host_sums1, b->h[1].p, b->n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

// ---- adaptive sampling: two half accumulators and a stopping rule (rt.h) -----
// list[cur]: the tiles still traced, n_active of them holding px_active
// pixels.  An evaluation (adapt_eval_kernel behind an odd step) writes
// list[cur ^ 1] and counts its length and pixels in state[2 * (gen & 1) ..];
// that pair is copied to `pinned` behind it, and the next step waits for `ev`
// and takes the two numbers from there: the grid of its launch depends on
// them.  The pairs alternate so that a kernel zeroes the one the evaluation
// after it counts in.  (samples: over all pixels, not per pixel.)
struct rt_adapt : HalfFrames {
  rt_adapt_opts opts{};
  DevBuf<int> list[2];
  DevBuf<unsigned> state;   // device u32[4]
  int step = 0, cur = 0, gen = 0;
  int n_active = 0;
  int64_t px_active = 0;
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
  rt_adapt* ad = nullptr;
  if (const int rc = halves_new("rt_adapt_create", *ds, *shape, &ad)) return rc;
  ad->opts = *opts;
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

extern "C" int rt_adapt_resolve(const rt_adapt* ad, int flags, float* d_out, void* hip_stream) {
  return halves_resolve("rt_adapt_resolve", ad, flags, d_out, nullptr, hip_stream);
}

extern "C" int rt_adapt_resolve_u8(const rt_adapt* ad, int flags, uint8_t* d_out, void* hip_stream) {
  return halves_resolve("rt_adapt_resolve_u8", ad, flags, nullptr, d_out, hip_stream);
}

extern "C" int rt_adapt_resolve_half(const rt_adapt* ad, int half, int flags, float* d_out, void* hip_stream) {
  return halves_resolve_half("rt_adapt_resolve_half", ad, half, flags, d_out, hip_stream);
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
  return halves_read("rt_adapt_read", ad, host_sums0, host_sums1, hip_stream);
}

// ---- the sample budget's frame (rt.h, budget.h) --------------
// mult per 8 x 8 tile of the output rows; list: every tile, by descending
// mult; state: the plan kernels' scratch; back: what the list kernel leaves
// for the host (n_j, px_j), copied to `pinned` behind it -- rt_budget_trace
// waits for `ev` and takes the grids of its launches from there.  units[h]:
// rt_budget_trace_fused's unit tables, n_tiles x max_mult entries per half,
// made by the first fused trace; n_units: the entries the current plan's fused
// trace wrote (-1: none since the plan).
struct rt_budget : HalfFrames {
  rt_budget_opts opts{};
  DevBuf<uint32_t> mult;
  DevBuf<int> list;
  DevBuf<unsigned> state, back;   // device u32[kBdState], u32[kBdBack]
  DevBuf<BdUnit> units[2];
  int n_units = -1;
  bool planned = false;   // a plan no trace has used yet
  bool have = false;      // nj, px hold a plan's numbers
  unsigned nj[kBdMaxMult] = {}, px[kBdMaxMult] = {};
};

extern "C" int rt_budget_create(const rt_dscene* ds, const rt_params* shape, const rt_budget_opts* opts,
                                rt_budget** out) {
  clear_error();
  if (out) *out = nullptr;
  if (!ds || !shape || !opts || !out) return set_error(RT_E_ARG, "rt_budget_create: NULL argument");
  if (const char* why = bd_opts_error(*opts)) return set_error(RT_E_ARG, std::string("rt_budget_create: ") + why);
  if (shape->tile_step != 0) return set_error(RT_E_ARG, "rt_budget_create: tile_step must be 0 (a contiguous band)");
  rt_budget* bd = nullptr;
  if (const int rc = halves_new("rt_budget_create", *ds, *shape, &bd)) return rc;
  bd->opts = *opts;
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
  if (const int rc = stream_on_device(who, stream, bd->device, "the scene")) return rc;
  if (bd->pending) HIP_TRY(hipEventSynchronize(bd->ev));   // (`pinned` is about to be written again)
  bd->pending = bd->planned = bd->have = false;
  bd->n_units = -1;
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

// rt_budget_trace's samples in two launches (rt.h): budget_units_kernel writes
// both halves' unit tables from the list, then one pass per half over its
// table, at the whole frame's spp = 2 max_mult half_spp, of which a unit is
// one block of half_spp.  The grids are the plan's sum of the n_j: the
// read-back rt_budget_trace waits for.
extern "C" int rt_budget_trace_fused(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_budget* bd,
                                     uint64_t* d_counters, void* hip_stream) {
  clear_error();
  if (!ds || !c || !p || !bd) return set_error(RT_E_ARG, "rt_budget_trace_fused: NULL argument");
  if (const int rc = check_match("rt_budget_trace_fused", "the budgeted frame", *bd, *ds, *p)) return rc;
  std::lock_guard<std::mutex> lk(bd->mu);
  if (!bd->planned) return set_error(RT_E_ARG, "rt_budget_trace_fused: no fresh plan (rt_budget_plan comes first)");
  const rt_budget_opts& o = bd->opts;
  if (p->sample_begin < 0 || static_cast<int64_t>(p->sample_begin) + 2ll * o.max_mult * o.half_spp > INT_MAX)
    return set_error(RT_E_ARG, "rt_budget_trace_fused: sample_begin + 2 * max_mult * half_spp passes 2^31 - 1");
  HIP_TRY(hipSetDevice(bd->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device("rt_budget_trace_fused", stream, bd->device, "the scene")) return rc;
  rt_params q = *p;
  q.spp = 2 * o.max_mult * o.half_spp;
  q.sample_begin = p->sample_begin;
  // (launch_impl's refusal, asked before the table kernel is enqueued: a refused call enqueues nothing)
  int vsel = 0;
  if (launch_tile_rows(*ds, q, &vsel) != kTile)
    return set_error(RT_E_ARG, "rt_budget_trace_fused: variant " + std::to_string(vsel) + " has no 8 x 8 tiles");
  if (const int rc = budget_settle(bd)) return rc;
  int64_t total = 0;
  for (int j = 0; j < o.max_mult; ++j) total += std::min<unsigned>(bd->nj[j], static_cast<unsigned>(bd->n_tiles));
  const int64_t cap = static_cast<int64_t>(bd->n_tiles) * o.max_mult;   // (halves_new: within an int)
  if (total <= 0 || total > cap) return set_error(RT_E_ARG, "rt_budget_trace_fused: the plan's counts do not add up");
  for (int h = 0; h < 2; ++h)
    if (!bd->units[h]) {
      HIP_TRY(bd->units[h].alloc(static_cast<size_t>(cap)));
      // (x = -1: no unit)
      HIP_TRY(hipMemsetAsync(bd->units[h].p, 0xff, static_cast<size_t>(cap) * sizeof(BdUnit), stream));
    }
  HIP_TRY(enqueue(budget_units_kernel, dim3(static_cast<unsigned>((bd->n_tiles + 255) / 256)), dim3(256), 0, stream,
                  static_cast<const int*>(bd->list.p), static_cast<const uint32_t*>(bd->mult.p),
                  static_cast<const unsigned*>(bd->back.p), bd->n_tiles, o.max_mult, static_cast<int>(cap),
                  bd->units[0].p, bd->units[1].p));
  bd->n_units = static_cast<int>(total);
  int launches = 0;
  for (int h = 0; h < 2; ++h) {
    if (const int rc = launch_impl(ds, c, &q, nullptr, d_counters, hip_stream, bd->h[h].p, "rt_budget_trace_fused",
                                   nullptr, 0, reinterpret_cast<const int2*>(bd->units[h].p), bd->n_units))
      return rc;
    ++launches;
  }
  bd->planned = false;
  return launches;
}

extern "C" int rt_budget_resolve(const rt_budget* bd, int flags, float* d_out, void* hip_stream) {
  return halves_resolve("rt_budget_resolve", bd, flags, d_out, nullptr, hip_stream);
}

extern "C" int rt_budget_resolve_half(const rt_budget* bd, int half, int flags, float* d_out, void* hip_stream) {
  return halves_resolve_half("rt_budget_resolve_half", bd, half, flags, d_out, hip_stream);
}

extern "C" int rt_budget_read(const rt_budget* bd, uint64_t* host_sums0, uint64_t* host_sums1, void* hip_stream) {
  return halves_read("rt_budget_read", bd, host_sums0, host_sums1, hip_stream);
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

extern "C" int rt_budget_list_read(const rt_budget* bd, int32_t* host_list, void* hip_stream) {
  clear_error();
  if (!bd || !host_list) return set_error(RT_E_ARG, "rt_budget_list_read: NULL argument");
  HIP_TRY(hipSetDevice(bd->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_list, bd->list.p, bd->n_tiles * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return RT_OK;
}

extern "C" int rt_budget_units_read(const rt_budget* bd, int half, int32_t* host_units, void* hip_stream) {
  clear_error();
  if (!bd || !host_units) return set_error(RT_E_ARG, "rt_budget_units_read: NULL argument");
  if (half != 0 && half != 1) return set_error(RT_E_ARG, "rt_budget_units_read: half is neither 0 nor 1");
  std::lock_guard<std::mutex> lk(bd->mu);
  if (bd->n_units < 0 || !bd->units[half])
    return set_error(RT_E_ARG, "rt_budget_units_read: no rt_budget_trace_fused since the plan");
  HIP_TRY(hipSetDevice(bd->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemcpyAsync(host_units, bd->units[half].p, static_cast<size_t>(bd->n_units) * sizeof(BdUnit),
                         hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return bd->n_units;
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
