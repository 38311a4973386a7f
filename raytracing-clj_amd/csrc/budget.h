// budget.h — the sample budget (rt_budget_*, include/rt.h):
// from a per-pixel history length (rt_temporal_probe) to one sample multiplier
// per 8 x 8 tile, so that a frame of compute-pixel's loop
// (src/raytracing.clj:141-155) spends its samples where the temporal history is
// short.
//
// Replaces nothing the reference computes: the reference traces every pixel at
// one rate; the plan only decides how many blocks of half_spp samples a tile's
// pixels get, each sample being the reference's own.
//
// Two parts, as denoise.h and temporal.h.
//  1. The rule as plain inline functions that compile for the device (the
//     plan kernel below) and for the host (rt_budget_plan_host): one tile's
//     multiplier from its counts of short pixels.  All in integers, so the
//     result cannot depend on the order of evaluation; the only float
//     operation is the comparison len >= float(j).  A tile hands the rule its
//     counts through a callable, so that the host may loop over the tile's
//     pixels and the device take a ballot.
//  2. The device kernels (under __HIPCC__ and RT_BUDGET_KERNEL): the plan (one
//     wave per tile, lane = pixel), the clamp of a caller's multipliers, the
//     list (the tiles by descending multiplier, the prefix counts and the
//     per-tile sample counts), and the fused trace's unit tables -- whose rule
//     is again one text for the device and for rt_budget_units_host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "denoise.h"

namespace rtclj {

constexpr int kBdTile = 8;        // rt_adapt's tiles
constexpr int kBdMaxMult = 16;    // rt.h's cap on max_mult (and the weighted step's on a weight)
constexpr int kBdMaxTarget = 32;

// nullptr, or which rule of rt.h's table the options break
inline const char* bd_opts_error(const rt_budget_opts& o) {
  if (o.half_spp < 1) return "half_spp < 1";
  if (o.target < 1 || o.target > kBdMaxTarget) return "target outside 1..32";
  if (o.max_mult < 1 || o.max_mult > kBdMaxMult) return "max_mult outside 1..16";
  if (o.quantile_64 < 1 || o.quantile_64 > 64) return "quantile_64 outside 1..64";
  if (2ll * o.max_mult * static_cast<int64_t>(o.half_spp) > RT_MAX_SPP) return "2 * max_mult * half_spp > RT_MAX_SPP";
  return nullptr;
}

// a pixel counts as short of j frames unless len >= float(j) (a NaN is short)
RT_DN_FN bool bd_short(float len, int j) { return !(len >= static_cast<float>(j)); }

// min(max(m, 1), max_mult) of a caller's multiplier
RT_DN_FN uint32_t bd_clamp(uint32_t m, int max_mult) {
  return m < 1u ? 1u : (m > static_cast<uint32_t>(max_mult) ? static_cast<uint32_t>(max_mult) : m);
}

// the pixels of tile (tx, ty) that lie inside a rows x width band
RT_DN_FN int bd_tile_px(int tx, int ty, int width, int rows) {
  const int w = width - tx * kBdTile, h = rows - ty * kBdTile;
  return (w < kBdTile ? w : kBdTile) * (h < kBdTile ? h : kBdTile);
}

// One tile's multiplier (rt.h's rule).  count(j) = c_j, the number of the
// tile's npx pixels short of j frames, asked for j = 1, 2, ... in order until
// the first that reaches the quantile.
template <class Count>
RT_DN_FN uint32_t bd_tile_mult(const Count& count, int npx, int target, int max_mult, int quantile_64) {
  for (int j = 1; j <= target; ++j) {
    if (count(j) * 64 >= quantile_64 * npx) {   // (at most 64 * 64)
      const int m = target - (j - 1);           // (>= 1: j <= target)
      return static_cast<uint32_t>(m < max_mult ? m : max_mult);
    }
  }
  return 1u;
}

// rt_budget_plan_host (rt.h): the checks, then every tile.  0, or RT_E_ARG with
// *why set.
inline int bd_host_plan(const rt_budget_opts* o, const float* len, int width, int rows, uint32_t* mult,
                        const char** why) {
  *why = nullptr;
  if (!o || !len || !mult) {
    *why = "NULL argument";
    return RT_E_ARG;
  }
  if ((*why = bd_opts_error(*o)) != nullptr) return RT_E_ARG;
  if (width <= 0 || rows <= 0 || static_cast<int64_t>(width) * rows > 0x7fffffffll) {
    *why = "bad width/rows";
    return RT_E_ARG;
  }
  const int gx = (width + kBdTile - 1) / kBdTile, gy = (rows + kBdTile - 1) / kBdTile;
  for (int ty = 0; ty < gy; ++ty)
    for (int tx = 0; tx < gx; ++tx) {
      const int x1 = (tx + 1) * kBdTile < width ? (tx + 1) * kBdTile : width;
      const int y1 = (ty + 1) * kBdTile < rows ? (ty + 1) * kBdTile : rows;
      auto count = [&](int j) {
        int c = 0;
        for (int y = ty * kBdTile; y < y1; ++y)
          for (int x = tx * kBdTile; x < x1; ++x) c += bd_short(len[static_cast<size_t>(y) * width + x], j) ? 1 : 0;
        return c;
      };
      mult[static_cast<size_t>(ty) * gx + tx] =
          bd_tile_mult(count, bd_tile_px(tx, ty, width, rows), o->target, o->max_mult, o->quantile_64);
    }
  return RT_OK;
}

// ---- the fused trace's unit table (rt_budget_trace_fused) ----
// One entry per (tile, pass j < mult[tile]) and half h: trace_kernel's explicit
// unit (KArgs::unit_tab) {x = tile, y = k | s << 8}, samples [k spp / s,
// (k + 1) spp / s) of the tile.  With spp = 2 max_mult half_spp, s = 2 max_mult
// and k = 2 j + h that is block k of half_spp samples: what pass j, half h of
// rt_budget_trace traces.  Block-major, in list order: pass 0's tiles, then
// pass 1's, ...; pass j's are the list's first n_j (it is sorted by descending
// multiplier), so list position i of pass j has slot sum_{j' < j} n_j' + i and
// the table is a function of the list alone.  (An int2's members; a host
// caller's array need not be 8-byte aligned.)
struct BdUnit {
  int32_t x, y;
};

// List position i holds `tile`, of multiplier m (1 .. max_mult): its entries of
// both halves' tables (either may be NULL), m each.  nj[j] = #{tiles with
// mult > j}; a slot at or past `cap` is not written (never, for a list in
// descending order and its own n_j: then i < n_j for every j < m).
RT_DN_FN void bd_units_at(int i, int tile, uint32_t m, const unsigned* nj, int max_mult, int cap, BdUnit* tab0,
                          BdUnit* tab1) {
  const int s = (2 * max_mult) << 8;
  int base = 0;   // sum_{j' < j} n_j'
  for (int j = 0; j < static_cast<int>(m) && j < max_mult; ++j) {
    const int slot = base + i;
    if (slot >= 0 && slot < cap) {
      if (tab0) tab0[slot] = BdUnit{tile, (2 * j) | s};
      if (tab1) tab1[slot] = BdUnit{tile, (2 * j + 1) | s};
    }
    base += static_cast<int>(nj[j]);
  }
}

// rt_budget_units_host (rt.h): the checks, the n_j from mult, then every list
// position.  The number of entries (the sum of the multipliers), or RT_E_ARG
// with *why set and nothing written.
inline int bd_host_units(const int32_t* list, const uint32_t* mult, int n_tiles, int max_mult, int half, int32_t* out,
                         const char** why) {
  *why = nullptr;
  if (!list || !mult || !out) {
    *why = "NULL argument";
    return RT_E_ARG;
  }
  if (max_mult < 1 || max_mult > kBdMaxMult) {
    *why = "max_mult outside 1..16";
    return RT_E_ARG;
  }
  if (half != 0 && half != 1) {
    *why = "half is neither 0 nor 1";
    return RT_E_ARG;
  }
  if (n_tiles <= 0 || n_tiles > 0x7fffffff / kBdMaxMult) {
    *why = "bad n_tiles";
    return RT_E_ARG;
  }
  unsigned nj[kBdMaxMult] = {};
  for (int t = 0; t < n_tiles; ++t) {
    if (mult[t] < 1u || mult[t] > static_cast<uint32_t>(max_mult)) {
      *why = "a multiplier outside 1..max_mult";
      return RT_E_ARG;
    }
    for (uint32_t j = 0; j < mult[t]; ++j) ++nj[j];
  }
  // the list: every tile once, by descending multiplier (nj[m] as the tile's
  // mark: positions [nj[m], nj[m - 1]) hold the tiles of multiplier m)
  for (int i = 0; i < n_tiles; ++i) {
    if (list[i] < 0 || list[i] >= n_tiles) {
      *why = "a list entry outside the tiles";
      return RT_E_ARG;
    }
    const uint32_t m = mult[list[i]];
    const unsigned lo = m < static_cast<uint32_t>(kBdMaxMult) ? nj[m] : 0u;
    if (static_cast<unsigned>(i) < lo || static_cast<unsigned>(i) >= nj[m - 1]) {
      *why = "the list is not in descending order of multiplier";
      return RT_E_ARG;
    }
  }
  std::vector<unsigned char> seen(static_cast<size_t>(n_tiles), 0);
  for (int i = 0; i < n_tiles; ++i) {
    if (seen[list[i]]) {
      *why = "a tile is listed twice";
      return RT_E_ARG;
    }
    seen[list[i]] = 1;
  }
  int total = 0;
  for (int j = 0; j < max_mult; ++j) total += static_cast<int>(nj[j]);
  BdUnit* tab = reinterpret_cast<BdUnit*>(out);
  for (int i = 0; i < n_tiles; ++i)
    bd_units_at(i, list[i], mult[list[i]], nj, max_mult, total, half == 0 ? tab : nullptr, half == 1 ? tab : nullptr);
  return total;
}

#if defined(__HIPCC__) && defined(RT_BUDGET_KERNEL)
// ------------------------------------------------------------- the kernels ----
// A plan's scratch, device u32[kBdState]: how many tiles took each multiplier
// and how many pixels they hold, and the list kernel's cursors.  Zeroed before
// the plan kernel.
constexpr int kBdHistN = 0, kBdHistPx = kBdMaxMult + 1, kBdCursor = 2 * (kBdMaxMult + 1), kBdState = 64;
// The read-back, u32[2 * kBdMaxMult]: n_j = #{tiles with mult > j}, then
// px_j = their pixels, j = 0 .. kBdMaxMult - 1.
constexpr int kBdBack = 2 * kBdMaxMult;

// `m` is tile `tile`'s multiplier (inside 1 .. max_mult <= kBdMaxMult): store
// it and count it.  One thread per tile calls this.
__device__ __forceinline__ void bd_commit(uint32_t* __restrict__ mult, unsigned* __restrict__ state, int tile, uint32_t m,
                                          int npx) {
  mult[tile] = m;
  __hip_atomic_fetch_add(&state[kBdHistN + m], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(&state[kBdHistPx + m], static_cast<unsigned>(npx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// rt_budget_plan: one wave per tile, lane = pixel (row lane / 8, column
// lane % 8, as adapt_eval_kernel's); a lane outside the band holds nothing.
// c_j is one ballot and a population count; the loop over j is uniform.
constexpr int kBdPlanWaves = 4;   // tiles per block
__global__ __launch_bounds__(64 * kBdPlanWaves) void budget_plan_kernel(const float* __restrict__ len, int width,
                                                                        int rows, int tiles_x, int n_tiles,
                                                                        int target, int max_mult, int quantile_64,
                                                                        uint32_t* __restrict__ mult,
                                                                        unsigned* __restrict__ state) {
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int tile = static_cast<int>(blockIdx.x) * kBdPlanWaves + (static_cast<int>(threadIdx.x) >> 6);
  if (tile >= n_tiles) return;   // (the whole wave)
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x = tx * kBdTile + (lane & 7), y = ty * kBdTile + (lane >> 3);
  const bool inside = x < width && y < rows;
  const float l = inside ? len[static_cast<size_t>(y) * width + x] : 0.0f;
  const int npx = __popcll(__ballot(inside));
  auto count = [&](int j) { return static_cast<int>(__popcll(__ballot(inside && bd_short(l, j)))); };
  const uint32_t m = bd_tile_mult(count, npx, target, max_mult, quantile_64);
  if (lane == 0) bd_commit(mult, state, tile, m, npx);
}

// rt_budget_plan_mult: the caller's multipliers clamped to 1 .. max_mult before
// anything indexes by them; a thread per tile.
__global__ __launch_bounds__(256) void budget_clamp_kernel(const uint32_t* __restrict__ in, int width, int rows,
                                                           int tiles_x, int n_tiles, int max_mult,
                                                           uint32_t* __restrict__ mult, unsigned* __restrict__ state) {
  const int tile = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (tile >= n_tiles) return;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  bd_commit(mult, state, tile, bd_clamp(in[tile], max_mult), bd_tile_px(tx, ty, width, rows));
}

// The list: the tiles by descending multiplier.  The tiles of multiplier m
// start at n_m = #{mult > m} (from the plan's counts) and take their places
// among themselves from an atomic cursor -- that order is whatever the atomics
// give, and no bit depends on it.  The list's first n_j tiles are then those
// with mult > j: pass j's.  Also counts[tile] = 2 * mult * half_spp, and by
// block 0 the read-back's n_j and px_j.  A thread per tile.
__global__ __launch_bounds__(256) void budget_list_kernel(const uint32_t* __restrict__ mult, int n_tiles, int half_spp,
                                                          unsigned* __restrict__ state, int* __restrict__ list,
                                                          uint32_t* __restrict__ counts, unsigned* __restrict__ back) {
  __shared__ unsigned s_base[kBdMaxMult + 1];   // s_base[m] = #{tiles with mult > m}, m = 0 .. kBdMaxMult
  if (threadIdx.x == 0) {
    unsigned n = 0u, px = 0u;
    for (int m = kBdMaxMult; m >= 0; --m) {
      s_base[m] = n;   // the tiles above m
      if (blockIdx.x == 0 && m < kBdMaxMult) {
        back[m] = n;
        back[kBdMaxMult + m] = px;
      }
      // (the counts were complete before this kernel started; this kernel adds to the cursors only)
      n += state[kBdHistN + m];
      px += state[kBdHistPx + m];
    }
  }
  __syncthreads();
  const int tile = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (tile >= n_tiles) return;
  const uint32_t m = mult[tile];   // (1 .. kBdMaxMult: bd_commit's)
  const unsigned at =
      s_base[m] + __hip_atomic_fetch_add(&state[kBdCursor + m], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (at < static_cast<unsigned>(n_tiles)) list[at] = tile;   // (always: the counts add up to n_tiles)
  counts[tile] = 2u * m * static_cast<uint32_t>(half_spp);
}

// rt_budget_trace_fused: both halves' unit tables (bd_units_at) from the list,
// the multipliers and the n_j the list kernel left in `back`.  A thread per
// list position; every slot below sum_j n_j is written by exactly one thread,
// none at or past `cap`.
__global__ __launch_bounds__(256) void budget_units_kernel(const int* __restrict__ list,
                                                           const uint32_t* __restrict__ mult,
                                                           const unsigned* __restrict__ back, int n_tiles, int max_mult,
                                                           int cap, BdUnit* __restrict__ tab0, BdUnit* __restrict__ tab1) {
  const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (i >= n_tiles) return;
  const int tile = list[i];
  if (tile < 0 || tile >= n_tiles) return;   // (never: the list holds tiles of the frame, always)
  bd_units_at(i, tile, mult[tile], back, max_mult, cap, tab0, tab1);
}
#endif  // __HIPCC__ && RT_BUDGET_KERNEL

}  // namespace rtclj
