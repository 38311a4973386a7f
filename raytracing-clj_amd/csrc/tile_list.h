// tile_list.h — which bodies the camera rays of one pixel rectangle can reach:
// a conservative cull, as plain inline functions that compile for the device
// (trace_kernel.h's workgroup prologue) and for the host
// (tools/tile_list_check.cpp, the CPU property test's driver): one text for
// both, as bvh_pad.h.
//
// The ray set.  A camera ray of the rectangle starts at
//   o = center + qx disk_u + qy disk_v,   |q| <= 1   (center without defocus)
// and aims at
//   f = p00 + fx du + fy dv,   fx in [x0 - 0.5, x1 + 0.5], fy in [y0 - 0.5, y1 + 0.5]
// (x0 .. x1, y0 .. y1: the rectangle's first and last pixel centres).  Its
// points are P(s) = o + s (f - o), s >= 0.
//
// The bound.  With c0 = center, f0 = f at the rectangle's centre and the axis
// A(s) = c0 + s (f0 - c0):  P(s) - A(s) = (1 - s)(o - c0) + s (f - f0), so
//   |P(s) - A(s)| <= rho(s) = |1 - s| R_l + s R_f,
// R_l bounding |o - c0| and R_f bounding |f - f0|:
//   |qx U + qy V|^2 <= max(|U|^2, |V|^2) |q|^2 + 2 |qx qy| |U.V| <= max(|U|^2, |V|^2) + |U.V|,
//   |a du + b dv|^2 <= hx^2 |du|^2 + hy^2 |dv|^2 + 2 hx hy |du.dv|   for |a| <= hx, |b| <= hy,
// hx = (x1 - x0) / 2 + 0.5, hy likewise.
//
// The body test (trace_kernel.h's leaf pass) makes body (C, r) a candidate
// when disc >= 0 and not (h < 0 and c >= 0): the line passes within r of C, and
// C lies ahead of the origin or the origin inside the body -- so some point
// P(s), s >= 0, is within r of C, up to the test's own error, which
// tools/pad_bound.cpp measures as 6e-4 (|oc| + r).  Hence a candidate has
//   |C - A(s)| <= r + rho(s) + m0 + s m1    for some s >= 0,
//   m0 = min(kTlRel M, (kTlRel M)^2 / (2 r)) + kTlAbs S,   M = |C - c0| + R_l + r >= |oc| + r
//   (kTlRel M: 3.3 x the measured error; the second form, for a body large
//   beside M such as the ground, from the candidate test itself: its disc,
//   h^2 - c, is off by a few 2^-24 M^2, far less than kTlRel^2 M^2, and
//   disc >= -e puts the line within sqrt(r^2 + e) <= r + e / (2 r) of C),
//   m1 = kTlAbs S,   S = |c0| + |f0| + R_l + R_f
// (the kTlAbs terms: o, f and f - o are rounded to fp32, up to 2e-7 of their
// coordinates' size, and the disk samplers reach |q| <= 1 + 1e-6; 4e-6 is a
// margin of 10 and more).  Both sides are positive and linear in s on [0, 1]
// and on [1, inf), so squared this is a quadratic inequality
//   q(s) = A s^2 - 2 B s + Cq <= 0
// per piece: true at an end of the piece, or, for A > 0, at the vertex B / A
// inside it.  On the finite piece a non-positive A leaves the ends (q concave
// or linear); on the infinite one it cannot be decided: the body is kept.
// Everything is computed in double from the fp32 inputs, so the cull's own
// rounding (1e-16) is nothing beside the margins; every comparison is written
// so that a NaN (a non-finite camera or body) keeps the body.
//
// A false positive costs a list entry; a false cull would break the frame:
// tools/tile_list_check.cpp counts them over millions of (ray, body) pairs.
#pragma once
#include <cmath>

#include "bvh.h"

#if defined(__HIPCC__)
#define RT_TL_FN __host__ __device__ __forceinline__
#else
#define RT_TL_FN inline
#endif

namespace rtclj {

constexpr double kTlRel = 2e-3;   // of |oc| + r: the body test's outward error, 6e-4 measured
constexpr double kTlAbs = 4e-6;   // of the camera's coordinate sizes: fp32 rounding of o, f, f - o

// the camera rays of a pixel rectangle: the axis and the radius terms
struct TileRays {
  double c[3], v[3];   // A(s) = c + s v
  double rl, rf;       // R_l; R_f + m1
  double mabs;         // kTlAbs S
};

// cam: center, p00, du, dv, disk_u, disk_v (KArgs::cam); x0 <= x1, y0 <= y1:
// the first and last pixel centres (columns; image rows).  rf_scale: 1 (the
// CPU check's negative control halves R_f)
RT_TL_FN TileRays tile_rays(const float* cam, int defocus, float x0, float x1, float y0, float y1, double rf_scale = 1.0) {
  TileRays t;
  const double fx = 0.5 * (static_cast<double>(x0) + x1), fy = 0.5 * (static_cast<double>(y0) + y1);
  const double hx = 0.5 * (static_cast<double>(x1) - x0) + 0.5, hy = 0.5 * (static_cast<double>(y1) - y0) + 0.5;
  double uu = 0, vv = 0, uv = 0, dudu = 0, dvdv = 0, dudv = 0, nc = 0, nf = 0;
  for (int k = 0; k < 3; ++k) {
    const double du = cam[6 + k], dv = cam[9 + k], U = defocus ? cam[12 + k] : 0.0, V = defocus ? cam[15 + k] : 0.0;
    const double f0 = cam[3 + k] + fx * du + fy * dv;
    t.c[k] = cam[k];
    t.v[k] = f0 - t.c[k];
    uu += U * U, vv += V * V, uv += U * V;
    dudu += du * du, dvdv += dv * dv, dudv += du * dv;
    nc += t.c[k] * t.c[k], nf += f0 * f0;
  }
  t.rl = sqrt((uu > vv ? uu : vv) + fabs(uv));
  const double rf = rf_scale * sqrt(hx * hx * dudu + hy * hy * dvdv + 2.0 * hx * hy * fabs(dudv));
  t.mabs = kTlAbs * (sqrt(nc) + sqrt(nf) + t.rl + rf);
  t.rf = rf + t.mabs;
  return t;
}

// can a camera ray of the rectangle make body (C, w = -r^2) a candidate of the
// body test?  false only when the bound above excludes it
RT_TL_FN bool tile_keeps(const TileRays& t, float cx, float cy, float cz, float w) {
  // a pad body (w = +inf: disc = -inf, never a candidate)
  if (w == INFINITY) return false;
  const double r = sqrt(-static_cast<double>(w));
  const double wx = cx - t.c[0], wy = cy - t.c[1], wz = cz - t.c[2];
  const double ww = wx * wx + wy * wy + wz * wz;
  const double wv = wx * t.v[0] + wy * t.v[1] + wz * t.v[2];
  const double vv = t.v[0] * t.v[0] + t.v[1] * t.v[1] + t.v[2] * t.v[2];
  // the test's error: kTlRel M, or for a body large beside M the tighter
  // kTlRel^2 M^2 / (2 r) (disc >= 0 with an error of eps M^2 puts the line
  // within sqrt(r^2 + eps M^2) <= r + eps M^2 / (2 r) of C; eps = kTlRel^2)
  const double M = sqrt(ww) + t.rl + r, e1 = kTlRel * M, e2 = e1 * e1 / (2.0 * r);
  const double K = r + (e2 < e1 ? e2 : e1) + t.mabs;
  // q(s) > 0 strictly, spelled so that a NaN reads "not excluded"
  auto excluded = [&](double a0, double a1, bool finite) {
    const double A = vv - a1 * a1, B = wv + a0 * a1, Cq = ww - a0 * a0;
    // the piece's ends: s = 0 | 1 for [0, 1]; s = 1 for [1, inf)
    const double q1 = A - 2.0 * B + Cq;
    if (!(q1 > 0.0)) return false;
    if (finite && !(Cq > 0.0)) return false;
    if (!(A > 0.0)) return finite && A <= 0.0;   // [0, 1]: concave or linear, the ends decide; [1, inf): kept
    const double sv = B / A;                     // the vertex, q(sv) = Cq - B^2 / A
    const bool inside = finite ? (sv > 0.0 && sv < 1.0) : sv > 1.0;
    if (!(sv == sv)) return false;
    if (inside && !(Cq - B * sv > 0.0)) return false;
    return true;
  };
  // [0, 1]: E(s) = (K + R_l) + s (R_f - R_l); [1, inf): E(s) = (K - R_l) + s (R_f + R_l)
  return !(excluded(K + t.rl, t.rf - t.rl, true) && excluded(K - t.rl, t.rf + t.rl, false));
}

// The list as the kernel holds it (trace_kernel.h: the prologue writes it, the
// prelude's trip reads it): a count word and up to kTlMax u16 entries, one per
// kept body.  A body is slot j of a leaf record of the 4-body tree: kTlRecBytes
// bytes, the four bodies as float4s (cx, cy, cz, -r^2) at + 16 j, their
// indices at + 64 + 4 j.  The records start 16-aligned and are a multiple of
// 16 long, so an address's two low bits are free: the entry is the record's
// address with j there.  More than kTlMax kept bodies, or a record above 64 KB:
// no list.
constexpr int kTlMax = 14;
constexpr unsigned kTlRecBytes = 80;
static_assert(kTlRecBytes % 16 == 0, "a record's address leaves its low bits to the slot");
RT_TL_FN unsigned tl_entry(unsigned rec_addr, unsigned j) { return rec_addr | j; }
RT_TL_FN unsigned tl_body_addr(unsigned e) { return (e & ~3u) + ((e & 3u) << 4); }
RT_TL_FN unsigned tl_index_addr(unsigned e) { return (e & ~3u) + 64u + ((e & 3u) << 2); }

// The pixel rectangle of 8 x th tile `tile` of a launch's compacted rows, as
// the kernel's prologue takes it: the first and last pixel centres (columns;
// image rows -- with interleaved row tiles, tile_step > 0, compacted row r is
// image row row_begin + (tile_first + (r / row_tile) tile_step) row_tile + r %
// row_tile).  false: the tile holds no pixel.
struct TlFrame {
  int width, rows_out, row_begin, row_tile, tile_first, tile_step;
};
inline bool tl_rect(const TlFrame& f, int th, int tile, float* x0, float* x1, float* y0, float* y1) {
  const int tiles_x = (f.width + 7) / 8;
  const int tby = tile / tiles_x, tbx = tile - tby * tiles_x;
  const int qx0 = tbx * 8, qy0 = tby * th;
  const int vw = f.width - qx0 < 8 ? f.width - qx0 : 8, vh = f.rows_out - qy0 < th ? f.rows_out - qy0 : th;
  if (vw <= 0 || vh <= 0) return false;
  auto image_row = [&](int r) {
    if (f.tile_step > 0) {
      const int t = r / f.row_tile;
      return f.row_begin + (f.tile_first + t * f.tile_step) * f.row_tile + (r - t * f.row_tile);
    }
    return f.row_begin + r;
  };
  *x0 = static_cast<float>(qx0), *x1 = static_cast<float>(qx0 + vw - 1);
  *y0 = static_cast<float>(image_row(qy0)), *y1 = static_cast<float>(image_row(qy0 + vh - 1));
  return true;
}

// The prologue's pass on the host (rt_tile_bodies_host): tile_keeps over every
// body of every leaf record -- pairs as bvh_build leaves them, 8 floats per
// pair (x0 x1 y0 y1 z0 z1 w0 w1), two pairs a record; pidx their body indices.
// bodies / slots (nullable) receive the first `cap` kept bodies' indices and
// places 4 record + j, in record order; returns how many are kept.
inline int tl_host_bodies(const TileRays& t, const float* pairs, const int* pidx, int n_rec, int* bodies, int* slots,
                          int cap) {
  int kept = 0;
  for (int k = 0; k < n_rec; ++k)
    for (int j = 0; j < 4; ++j) {
      const int pr = 2 * k + (j >> 1), e = j & 1;
      const float* p = pairs + 8 * static_cast<long>(pr);
      if (!tile_keeps(t, p[e], p[2 + e], p[4 + e], p[6 + e])) continue;
      if (kept < cap) {
        if (bodies) bodies[kept] = pidx[2 * pr + e];
        if (slots) slots[kept] = 4 * k + j;
      }
      ++kept;
    }
  return kept;
}

// rt_tile_bodies_host's body (and tools/tile_bodies_check.cpp's subject): the
// 4-body tree of the scene as rt_scene_upload builds it, the tile's rectangle,
// the pass above.  sphere: n x (cx, cy, cz, r); cam: KArgs::cam's 18 floats.
inline int tl_host_tile(const float* sphere, int n, bool sah, const float* cam, int defocus, const TlFrame& f, int tile,
                        int* bodies, int* slots, int cap) {
  float x0, x1, y0, y1;
  if (!tl_rect(f, 8, tile, &x0, &x1, &y0, &y1)) return 0;
  BvhHost tree;
  bvh_build(sphere, n, &tree, 4, sah);
  const TileRays t = tile_rays(cam, defocus, x0, x1, y0, y1);
  return tl_host_bodies(t, tree.pairs.data(), tree.pidx.data(), static_cast<int>(tree.pairs.size() / 16), bodies, slots, cap);
}

}  // namespace rtclj
