// variant_policy.h — which kernel variant a launch runs and the LDS it needs,
// as pure functions of a scene's three trees and the frame: integer
// arithmetic, no HIP, no environment, no state (trace.hip reads the selector,
// the RTCLJ_* knobs and the device's occupancy and passes them in).  Built
// for the host too: tools/variant_check.cpp runs it over
// tests/golden/variant_policy.json (tests/test_variant_policy.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "bvh.h"   // kBvhStack

namespace rtclj {
namespace policy {

// The kernels' shapes the policy sizes by (trace_kernel.h, first_hit.h;
// trace.hip and first_hit.hip assert that they are the kernels')
constexpr int kTile = 8;
constexpr int kPoolPx = kTile * kTile;
constexpr size_t kXBytes = 8 * 11 * 64 * 4;   // the sorted kernel's exchange buffer
constexpr int kFeatThreads = 256;
enum { FEAT_LDS = 0, FEAT_GLOBAL = 1, FEAT_SCAN = 2 };   // where a feature launch's bodies come from

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
//      -- camera segments resolved against a per-tile body list in a prelude
//      of the wave iteration, not by the walk (tile_list.h)
//   30 22 without the tile list (every segment through the walk: 22 as it was
//      before the list; selected only explicitly, for A/B and the tests that
//      hold the list path to the walk bit for bit)
//   18 BVH in LDS, 8-body leaves (large scenes where 24 does not fit)
//   12 BVH (2-body leaves) read from global memory: a tree too big for LDS
//    5 linear scan, grouped, table through the scalar cache: a tree too deep
//    0 = default (22 where it applies, else 16; 26, 24, else 18, when the 4-body tree's LDS image is large)
// The diagnostic library (lib/librtclj_diag.so) adds, from trace_diag.hip, the
// A/B variants -- 1, 2 simple scan (LDS, scalar cache), 4 grouped scan in LDS
// (north_star's LDS-staged scan), 8, 9 packed pairs, 11 BVH with 2-body leaves
// in LDS, 20 / 21 direction-coherent waves (sorted_kernel) -- and the
// statistics builds 3, 6, 7, 10, 13, 17 (= 16 + stats), 19 (= 18 + stats),
// 31 (= 22 + stats: the list path with the prelude's counters).
// Every variant renders the same bits.
enum : int {
  kDefault = 0,
  kScan = 5,          // linear scan: a tree too deep for the stack
  kGlobal = 12,       // 2-body leaves read from global memory: a tree too big for LDS
  kFull4 = 16,        // 4-body leaves, the full image
  kLeaf8 = 18,        // 8-body leaves
  kCompact = 22,      // 4-body leaves, the compact image
  kCompactW8 = 24,    // ... in 8-wave workgroups
  kCompactW16 = 26,   // ... in 16-wave workgroups
  kCompactTh4 = 28,   // ... on 8 x 4-pixel pools
  kCompactWalk = 30,  // ... without the per-tile list: camera segments through the walk
  kVariants = 32
};

enum { WALK_NONE = 0 /* a body scan */, WALK_BVH = 1, WALK_SORTED = 2 /* sorted_kernel */ };
enum { BUILD_NONE = 0, BUILD_PRODUCT = 1, BUILD_DIAG = 2 /* lib/librtclj_diag.so only */ };

// A variant without its kernel (trace.hip's variant_fn, trace_diag.hip's
// diag_kernel).  scan .. entry_bytes: what trace_kernel.h's traits say of the
// scan (trace.hip asserts it row by row).
struct Traits {
  int scan;      // SCAN_*
  int threads;   // workgroup size
  int th;        // the pool's tile rows (0: tile_rows(scan))
  bool lds;      // bodies or tree staged in LDS
  bool stats;    // a statistics build
  int build;     // BUILD_*
  int walk;      // WALK_*
  int tree;      // scan_tree: 0 = 2-body leaves, 1 = 4, 2 = 8
  bool compact;  // is_compact_scan: u8 node-index stack, u32 sums
  int entry_bytes;   // stack_entry_bytes
  int stats_build;   // the variant's statistics build in the diagnostic library (0: none)
};
constexpr Traits kNone{0, 256, 0, false, false, BUILD_NONE, WALK_NONE, 0, false, 2, 0};
constexpr Traits kTraits[kVariants] = {
    // scan thr th  lds    stats  build          walk         tree compact eb stats_build
    {5, 256, 0, true, false, BUILD_PRODUCT, WALK_BVH, 1, false, 2, 0},    //  0: resolved per scene (16's kernel)
    {0, 256, 0, true, false, BUILD_DIAG, WALK_NONE, 0, false, 2, 3},      //  1 simple scan, LDS
    {0, 256, 0, false, false, BUILD_DIAG, WALK_NONE, 0, false, 2, 0},     //  2 simple scan, scalar cache
    {0, 256, 0, true, true, BUILD_DIAG, WALK_NONE, 0, false, 2, 0},       //  3 = 1 + stats
    {1, 256, 0, true, false, BUILD_DIAG, WALK_NONE, 0, false, 2, 6},      //  4 grouped scan, LDS
    {1, 256, 0, false, false, BUILD_PRODUCT, WALK_NONE, 0, false, 2, 7},  //  5 grouped scan, scalar cache
    {1, 256, 0, true, true, BUILD_DIAG, WALK_NONE, 0, false, 2, 0},       //  6 = 4 + stats
    {1, 256, 0, false, true, BUILD_DIAG, WALK_NONE, 0, false, 2, 0},      //  7 = 5 + stats
    {2, 256, 0, true, false, BUILD_DIAG, WALK_NONE, 0, false, 2, 0},      //  8 packed pairs, LDS
    {2, 256, 0, false, false, BUILD_DIAG, WALK_NONE, 0, false, 2, 10},    //  9 packed pairs, scalar cache
    {2, 256, 0, false, true, BUILD_DIAG, WALK_NONE, 0, false, 2, 0},      // 10 = 9 + stats
    {3, 256, 0, true, false, BUILD_DIAG, WALK_BVH, 0, false, 2, 13},      // 11 BVH, 2-body leaves, LDS
    {3, 256, 0, false, false, BUILD_PRODUCT, WALK_BVH, 0, false, 2, 0},   // 12 ... global memory
    {3, 256, 0, true, true, BUILD_DIAG, WALK_BVH, 0, false, 2, 0},        // 13 = 11 + stats
    kNone,                                                                // 14 (dropped: while-while traversal)
    kNone,                                                                // 15 (dropped: its stats build)
    {5, 256, 0, true, false, BUILD_PRODUCT, WALK_BVH, 1, false, 2, 17},   // 16
    {5, 256, 0, true, true, BUILD_DIAG, WALK_BVH, 1, false, 2, 0},        // 17 = 16 + stats
    // (8-wave workgroups: one tree image for twice the waves)
    {6, 512, 0, true, false, BUILD_PRODUCT, WALK_BVH, 2, false, 1, 19},   // 18
    {6, 512, 0, true, true, BUILD_DIAG, WALK_BVH, 2, false, 1, 0},        // 19 = 18 + stats
    // direction-coherent waves (A/B, measured slower: profiles/r04/sorted_waves/):
    // octant-sorted, and lock-step packing only
    {7, 512, 0, true, false, BUILD_DIAG, WALK_SORTED, 1, false, 2, 0},    // 20
    {7, 512, 0, true, false, BUILD_DIAG, WALK_SORTED, 1, false, 2, 0},    // 21
    {8, 256, 0, true, false, BUILD_PRODUCT, WALK_BVH, 1, true, 1, 0},     // 22
    kNone,
    // (22's image in 8-wave workgroups: one tree image per 8 waves, for trees
    // too big for 22's 4-wave workgroups)
    {8, 512, 0, true, false, BUILD_PRODUCT, WALK_BVH, 1, true, 1, 0},     // 24
    kNone,
    // (and in 16-wave workgroups, 64 VGPRs: 8 waves per SIMD)
    {8, 1024, 0, true, false, BUILD_PRODUCT, WALK_BVH, 1, true, 1, 0},    // 26
    kNone,
    // (22 on 8 x 4-pixel pools: whole pools of half the pixels for launches of
    // few 8 x 8 tiles instead of sample splits; measured slower)
    {8, 256, 4, true, false, BUILD_PRODUCT, WALK_BVH, 1, true, 1, 0},     // 28
    kNone,
    // (22 without the tile list: camera segments through the walk)
    {8, 256, 0, true, false, BUILD_PRODUCT, WALK_BVH, 1, true, 1, 0},     // 30
    // (22's statistics build, the prelude's counters included: rt_debug_stats 27-31, rt_debug_stats_ext 32)
    {8, 256, 0, true, true, BUILD_DIAG, WALK_BVH, 1, true, 1, 0},         // 31 = 22 + stats
};
// does a build (diag: the diagnostic library) carry variant v?
constexpr bool has_variant(int v, bool diag) {
  return v >= 0 && v < kVariants && (kTraits[v].build == BUILD_PRODUCT || (diag && kTraits[v].build == BUILD_DIAG));
}
constexpr const Traits& traits(int v, bool diag) { return has_variant(v, diag) ? kTraits[v] : kNone; }
constexpr int variant_rows(const Traits& t) { return t.th ? t.th : t.walk == WALK_SORTED ? 16 : kTile; }

// What the policy reads of a scene on the device, and of a launch's frame
struct Tree {
  int n_nodes, depth, blob_f4;
};
struct Scene {
  Tree tree[3];   // 2-, 4-, 8-body leaves
  int n_pad;
  bool unit_albedo;
};
struct Frame {
  int width, height, rows, spp;
};

// traversal stack bytes: u8 entries for the 8-body-leaf tree (tree[2], at
// most 256 nodes when its variant runs), u16 otherwise
inline int stack_entries(const Tree& t, int tree) { return tree == 0 ? t.depth + 2 : std::max(t.depth, 1); }
// (threads: the workgroup's lanes, a stack row each)
inline size_t stack_of(const Tree& t, int tree, int threads = 256) {
  return static_cast<size_t>(stack_entries(t, tree)) * threads * (tree == 2 ? 1 : 2);
}
inline size_t lds_of(const Tree& t, int tree, int threads = 256) {
  return static_cast<size_t>(t.blob_f4) * 16 + stack_of(t, tree, threads);
}
// variant 22 (the compact image): u8 node indices, depth rows (the dead
// far-child write goes one above the top, as in 16)
inline int stack_entries_compact(const Tree& t) { return std::max(t.depth, 1); }
inline size_t lds_of_compact(const Tree& t, int threads) {
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

// selector -> the variant a launch on ds runs.  The order matters: a fallback
// can trigger the next (19 -> 17 -> 12 -> 5).
inline int resolve_variant(const Scene& ds, int vsel, bool diag) {
  const auto tr = [diag](int v) -> const Traits& { return traits(v, diag); };
  // default: 4-body leaves, unless that tree's LDS image limits a CU below
  // 5 workgroups (160 KB / 5) and the 8-body-leaf tree's is smaller
  // (measured: 1025 bodies 12.9 vs 14.0 ms; 484: 10.8 vs 12.2); each image
  // with the stack rows of its own variant's workgroup (18: 512 lanes)
  if (vsel == kDefault)
    vsel = (lds_of(ds.tree[1], 1) > kLds5 && ds.tree[2].n_nodes <= 256 &&
            lds_of(ds.tree[2], 2, tr(kLeaf8).threads) < lds_of(ds.tree[1], 1)) ? kLeaf8 : kFull4;
  // the 8-body walk (18, 19) -> the full 4-body one (16, 17).  u8 stack: 256 nodes at most
  if (tr(vsel).tree == 2 && ds.tree[2].n_nodes > 256) vsel = tr(vsel).stats ? tr(kFull4).stats_build : kFull4;
  // u16 stack of node LDS addresses: the kernel's static LDS (< 4 KB; 8 KB
  // allowed for) plus the node region must stay below 64 KB
  if (tr(vsel).walk == WALK_BVH && tr(vsel).tree == 1 && !tr(vsel).compact && ds.tree[1].n_nodes * 80 + 8192 > 65535)
    vsel = kGlobal;
  // the sorted kernels: the 4-body tree's byte-offset refs in a u16 stack
  // inside a wave's exchange slots, the blob beside the exchange buffer
  if (tr(vsel).walk == WALK_SORTED &&
      (ds.tree[1].n_nodes * 80 > 65535 || ds.tree[1].depth + 2 > kBvhStack ||
       static_cast<size_t>(ds.tree[1].blob_f4) * 16 + kXBytes > 96 * 1024))
    vsel = kFull4;
  if (tr(vsel).walk != WALK_NONE) {
    const int tree = tr(vsel).tree;
    const Tree& t = ds.tree[tree];
    if (t.depth + 2 > kBvhStack) return kScan;                       // tree too deep for the stack
    // (the stack rows of the variant's own workgroup size, as launch_lds)
    if (tr(vsel).lds && lds_of(t, tree, tr(vsel).threads) > 96 * 1024)
      vsel = kGlobal;   // tree too big for LDS: 2-body leaves, global
    if (!tr(vsel).lds && ds.tree[0].depth + 2 > kBvhStack) return kScan;   // (12: tree 0)
  }
  if (tr(vsel).compact && ds.tree[1].n_nodes > 256) vsel = kFull4;   // (u8 node indices)
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
inline bool compact_ok(const Scene& ds, const Frame& p) {
  return ds.unit_albedo && ds.tree[1].n_nodes <= 256 && p.spp < 65536 && ds.tree[1].depth + 2 <= kBvhStack &&
         p.width <= 65536 && p.height <= 65536;
}
// th4_ratio: RTCLJ_TH4; slots: the workgroups of 22 the device holds at once
// (read only where th4_ratio > 0)
inline int launch_variant(const Scene& ds, const Frame& p, int sel, bool diag, int th4_ratio, int slots) {
  const auto tr = [diag](int v) -> const Traits& { return traits(v, diag); };
  int vsel = resolve_variant(ds, sel, diag);
  if ((sel == kDefault && vsel == kFull4) || vsel == kCompact) vsel = compact_ok(ds, p) ? kCompact : kFull4;
  // A scene the default sends to the 8-body-leaf walk (its 4-body image too
  // big for five 4-wave workgroups a CU) runs 22's compact image on the
  // 4-body walk's leaf records instead, in workgroups that share one image
  // among more waves: 16-wave workgroups (26) where two fit a CU -- 8 waves
  // per SIMD in 64 VGPRs -- else 8-wave ones (24) where three fit -- 6 per
  // SIMD, as 18.  C4: 4.295 s (26) vs 4.570 (24) vs 4.931 (18), same boxes
  // (profiles/r05/c4_v26/, c4_v24/); C2's frame on 26 instead of 22: 260.4 vs
  // 251.8 ms (a pool's 32,000 samples over 1,024 lanes drain too often).
  if (sel == kDefault && vsel == kLeaf8 && compact_ok(ds, p)) {
    if (lds_of_compact(ds.tree[1], tr(kCompactW16).threads) + kStaticLds8 <= 160 * 1024 / 2)
      vsel = kCompactW16;
    else if (lds_of_compact(ds.tree[1], tr(kCompactW8).threads) + kStaticLds8 <= 160 * 1024 / 3)
      vsel = kCompactW8;
  }
  if (tr(vsel).compact && !compact_ok(ds, p)) vsel = kFull4;   // (an explicit 24, 26 or 28)
  // RTCLJ_TH4=r (A/B knob, default 0 = never): a launch of 22 with fewer
  // 8 x 8 tiles than r x the workgroups the device holds -- a shard of a
  // multi-GPU frame -- runs 28: the same image on 8 x 4-pixel pools, whole,
  // where 22 splits every tile's samples over 2-3 workgroups.  Measured at r
  // = 2 (profiles/r06/th4/): C1's 8-rank shard 1.62 ms against 0.84 with the
  // splits, the 4-rank 1.56 against 1.37 (the whole 8 x 4 pools are 1.84
  // rounds of 3,200-sample units: the last round's long units are the tail),
  // and 28 costs 5 % more per sample on the whole C1 frame (4.95 vs 4.71 ms:
  // a pool of half the pixels drains twice as often).  DESIGN.md §6.
  if (sel == kDefault && vsel == kCompact && th4_ratio > 0) {
    const int64_t n8 = static_cast<int64_t>((p.width + kTile - 1) / kTile) * ((p.rows + kTile - 1) / kTile);
    if (slots > 0 && n8 < static_cast<int64_t>(th4_ratio) * slots) vsel = kCompactTh4;
  }
  return vsel;
}

// dynamic LDS of a launch of variant vsel on ds
inline size_t launch_lds(const Scene& ds, int vsel, bool diag) {
  const Traits& v = traits(vsel, diag);
  if (v.walk == WALK_SORTED) return static_cast<size_t>(ds.tree[1].blob_f4) * 16 + kXBytes;   // blob | exchange
  if (v.compact) return lds_of_compact(ds.tree[1], v.threads);
  if (v.walk == WALK_BVH) {
    const Tree& t = ds.tree[v.tree];
    return v.lds ? lds_of(t, v.tree, v.threads) : stack_of(t, v.tree, v.threads);
  }
  return v.lds ? static_cast<size_t>(ds.n_pad) * 16 : 0;   // (the padded bodies, a float4 each)
}
// entries per lane: the ordered traversal (trees 1, 2) holds at most depth
// (a node on level L has L - 1 ancestors; the dead far-child write goes one
// above them); tree 0 also serves the while-while variants (depth + 2)
inline int launch_stack(const Scene& ds, const Traits& v) {
  return v.compact ? stack_entries_compact(ds.tree[v.tree]) : stack_entries(ds.tree[v.tree], v.tree);
}

// Where a feature launch on ds takes its bodies from, classed as
// resolve_variant classes the path kernel's variants: the selector's scan
// variants (5, the diagnostic 1-10) and a tree too deep for the stack give the
// linear scan; 12, or a tree image beyond the LDS budget, the tree in global
// memory; everything else the tree in LDS.  The tree is the 4-body-leaf one
// (tree[1]): half the nodes of the 2-body tree, and int body indices (the
// 8-body tree's are u16).  Budget: blob + stack rows within 160 KB / 5 less
// the kernel's 3.6 KB of static LDS, five workgroups per CU.
constexpr size_t kFeatLdsBudget = 160 * 1024 / 5 - 4096;
inline int feat_stack_rows(const Tree& t) { return t.depth + 1; }
inline size_t feat_stack_bytes(const Tree& t) { return static_cast<size_t>(feat_stack_rows(t)) * kFeatThreads * 2; }
inline int feat_source(const Scene& ds, int vsel, bool diag) {
  const Traits& v = traits(resolve_variant(ds, vsel, diag), diag);
  const Tree& t = ds.tree[1];
  if (v.walk == WALK_NONE || t.depth + 2 > kBvhStack) return FEAT_SCAN;
  if (!v.lds || static_cast<size_t>(t.blob_f4) * 16 + feat_stack_bytes(t) > kFeatLdsBudget) return FEAT_GLOBAL;
  return FEAT_LDS;
}
inline size_t feat_lds(const Scene& ds, int src) {
  const Tree& t = ds.tree[1];
  return src == FEAT_SCAN ? 0 : feat_stack_bytes(t) + (src == FEAT_LDS ? static_cast<size_t>(t.blob_f4) * 16 : 0);
}

// Where a body-id launch on ds (body_ids.h, rt_launch_ids) takes its bodies
// from: a feature launch's source and LDS (the same tree, the same stack rows
// for the same 256 lanes).  A workgroup traces one ray a thread here, against
// 64 x spp of feat_kernel, and stages the same image; staging still wins on
// C1's frame -- 19.8 us with the tree in LDS, 27.6 us with it in global memory
// (tools/motion_time.py) -- so the default is the feature
// pass's.
inline int ids_source(const Scene& ds, int vsel, bool diag) { return feat_source(ds, vsel, diag); }

// Sample split (rt_launch): split every tile of a launch with fewer tiles
// than kSplitRounds (RTCLJ_SPLIT_ROUNDS, default 3) x (resident workgroups), into enough splits to reach that
// (at most kSplitMax).  tools/shard_time.py on C1's 1/2/4/8-GPU shards
// (profiles/r02/shard_split_rounds.txt): 3-4 rounds best (8 GPUs: 5.88x at 3,
// 5.72x at 4, 5.30x at 6, 3.96x at 16; unsplit 2.57x)
constexpr int kSplitMax = 64;   // the most splits of one tile
// forced: RTCLJ_SPLIT (0: unset); slots: the workgroups the device holds at
// once; rounds: RTCLJ_SPLIT_ROUNDS (28: RTCLJ_TH4_SPLIT_ROUNDS); streamed:
// RT_FLAG_STREAMED.  For a launch with spp > 1.
inline int choose_split(int n_tiles, int spp, int forced, int slots, int rounds, bool streamed) {
  int split = 1;
  if (forced > 0) {
    split = forced;
  } else {
    const int64_t want = static_cast<int64_t>(rounds) * slots;
    if (slots > 0 && n_tiles < want) {
      split = static_cast<int>((want + n_tiles - 1) / n_tiles);
      // frames in flight: the next frame fills this launch's tail, so two
      // rounds of workgroups suffice (at least 2 splits: an unsplit heavy
      // tile would outlive two frames).  C1's 8-GPU shard, 2 streams:
      // 0.817 ms per frame at split 2 vs 0.87 at 3 (profiles/r03/shard_matrix_*.txt)
      if (streamed) split = std::max(2, static_cast<int>((2 * static_cast<int64_t>(slots) + n_tiles - 1) / n_tiles));
    }
  }
  return std::min(split, std::min(spp, kSplitMax));
}

}  // namespace policy
}  // namespace rtclj
