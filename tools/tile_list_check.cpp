// tile_list_check.cpp — CPU property check of the per-tile body list, on the
// text the kernel runs (raytracing-clj_amd/csrc/tile_list.h, host build).
//
// For random cameras and scenes it walks every tile of a small frame (partial
// border tiles included; tile heights 1 and 8), makes the tile's list with
// tile_rays / tile_keeps, generates camera rays of the tile by the kernel's
// fp32 camera arithmetic (trace_kernel.h: the jitter's extremes -0.5 and
// 0.5 - 2^-24, and +0.5; lens samples on the unit circle, inside it and at its
// centre) and runs the scan's fp32 body test on every body.  Every body that
// is a candidate of a ray -- disc >= 0 and not (h < 0 and c >= 0), the leaf
// pass's test -- must be in the list: a miss is a false cull, a hit the walk
// reports and the list path would lose.
//
// Cameras: no defocus, a small aperture, an aperture as large as the focus
// distance, far away from the origin (fp32 rounding of the camera sample).
// Bodies: in view, behind the camera, around the camera (the camera inside),
// tangent to an extreme ray of a tile (just inside and just outside), far
// smaller and far larger than a pixel.
//
// The negative control: the same run with R_f halved must report misses, or
// the cases would not reach the bound.
//
// Then C1's frame (cover(11), 1200 x 675, the cover camera): the list length
// over all 12,750 tiles, in bodies and in the 4-body tree's leaf records.
// Prints one JSON line; exit status 1 on any miss (or a control without one).
//
// g++ -O2 -std=c++17 -ffp-contract=off -mfma tools/tile_list_check.cpp csrc/bvh.cpp csrc/scenes.cpp
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../include/rt.h"
#include "../raytracing-clj_amd/csrc/bvh.h"
#include "../raytracing-clj_amd/csrc/tile_list.h"

using namespace rtclj;

namespace {

struct Body {
  float c[3], w;   // centre, -r^2 (the kernel's geo entry)
};
Body body(double x, double y, double z, double r) {
  const float rf = static_cast<float>(r);
  return {{static_cast<float>(x), static_cast<float>(y), static_cast<float>(z)}, -(rf * rf)};
}

// rt_camera_setup's arithmetic (raytracing.clj:117-139), in double, rounded once
void make_cam(int w, int h, double vfov, const double lf[3], const double la[3], double defocus_angle, double focus,
              float cam[18], int* defocus) {
  const double pi = 3.141592653589793;
  const double hh = std::tan(vfov * pi / 360.0), vh = 2.0 * hh * focus, vw = vh * (static_cast<double>(w) / h);
  double W[3] = {lf[0] - la[0], lf[1] - la[1], lf[2] - la[2]};
  const double wl = std::sqrt(W[0] * W[0] + W[1] * W[1] + W[2] * W[2]);
  for (double& x : W) x /= wl;
  double U[3] = {W[2], 0.0, -W[0]};   // up (0, 1, 0) x w
  const double ul = std::sqrt(U[0] * U[0] + U[2] * U[2]);
  for (double& x : U) x /= ul;
  const double V[3] = {W[1] * U[2] - W[2] * U[1], W[2] * U[0] - W[0] * U[2], W[0] * U[1] - W[1] * U[0]};
  const double rad = focus * std::tan(defocus_angle * pi / 360.0);
  for (int k = 0; k < 3; ++k) {
    const double du = U[k] * vw / w, dv = -V[k] * vh / h;
    const double corner = lf[k] - W[k] * focus - U[k] * vw / 2 + V[k] * vh / 2;
    cam[k] = static_cast<float>(lf[k]);
    cam[3 + k] = static_cast<float>(corner + 0.5 * (du + dv));
    cam[6 + k] = static_cast<float>(du);
    cam[9 + k] = static_cast<float>(dv);
    cam[12 + k] = static_cast<float>(U[k] * rad);
    cam[15 + k] = static_cast<float>(V[k] * rad);
  }
  *defocus = defocus_angle > 0 ? 1 : 0;
}

struct Ray {
  float o[3], d[3];
};
// one camera sample (trace_kernel.h's camera block): pixel (px, py) + jitter, lens sample q
Ray camera_ray(const float* cam, int defocus, float px, float py, float jx, float jy, float qx, float qy) {
  const float fx = px + jx, fy = py + jy;
  Ray r;
  float s[3];
  for (int k = 0; k < 3; ++k) s[k] = std::fmaf(cam[9 + k], fy, std::fmaf(cam[6 + k], fx, cam[3 + k]));
  for (int k = 0; k < 3; ++k)
    r.o[k] = defocus ? std::fmaf(cam[15 + k], qy, std::fmaf(cam[12 + k], qx, cam[k])) : cam[k];
  for (int k = 0; k < 3; ++k) r.d[k] = s[k] - r.o[k];
  return r;
}
// the leaf pass's candidate test of one body (the scan's op sequence)
bool candidate(const Ray& r, const float u[3], const Body& b) {
  const float ocx = b.c[0] - r.o[0], ocy = b.c[1] - r.o[1], ocz = b.c[2] - r.o[2];
  const float h = std::fmaf(u[2], ocz, std::fmaf(u[1], ocy, u[0] * ocx));
  const float c = std::fmaf(ocx, ocx, std::fmaf(ocz, ocz, std::fmaf(ocy, ocy, b.w)));
  const float disc = std::fmaf(h, h, -c);
  return disc >= 0.0f && !(h < 0.0f && c >= 0.0f);
}

struct Counts {
  long tiles = 0, rays = 0, pairs = 0, candidates = 0, misses = 0, control_misses = 0, kept = 0, bodies = 0;
  long no_defocus = 0, wide_aperture = 0, inside = 0, behind = 0, tangent = 0, tiny = 0, huge = 0, rows1 = 0, partial = 0;
};

// the rays of one tile: every pixel, jitter extremes and lens extremes
template <class F>
void tile_rays_each(const float* cam, int defocus, int x0, int x1, const std::vector<float>& rows, std::mt19937& g,
                    F&& f) {
  static const float jit[3] = {-0.5f, 0.5f - 0x1p-24f, 0.5f};
  std::uniform_real_distribution<float> U(-1.0f, 1.0f);
  for (float py : rows)
    for (int px = x0; px <= x1; ++px)
      for (int s = 0; s < 12; ++s) {
        const float jx = s < 9 ? jit[s % 3] : 0.5f * U(g), jy = s < 9 ? jit[s / 3] : 0.5f * U(g);
        float qx = 0, qy = 0;
        if (defocus) {
          const int m = (s * 7 + px) % 10;
          if (m < 8) {   // on the unit circle
            const float a = 0.785398163f * static_cast<float>(m) + 0.3f * U(g);
            qx = std::cos(a), qy = std::sin(a);
          } else if (m == 8) {
            qx = 0.7f * U(g), qy = 0.7f * U(g);
          }
        }
        f(camera_ray(cam, defocus, static_cast<float>(px), py, jx, jy, qx, qy));
      }
}

void run_case(std::mt19937& g, Counts& n) {
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto sym = [&](double a) { return a * (2.0 * U(g) - 1.0); };
  const int w = 9 + static_cast<int>(U(g) * 28), h = 5 + static_cast<int>(U(g) * 16);
  const int th = U(g) < 0.3 ? 1 : 8;
  const int step = U(g) < 0.4 ? 2 : 0;   // interleaved 1-row shards: a tile's rows 2 image rows apart
  const int kind = static_cast<int>(U(g) * 4);      // 0 no defocus, 1 small, 2 aperture ~ focus distance, 3 far from the origin
  const double shift = kind == 3 ? 1000.0 : 0.0;
  const double lf[3] = {sym(8) + shift, sym(4) + 1.0, sym(8) + shift};
  double la[3] = {sym(3) + shift, sym(1), sym(3) + shift};
  if (std::fabs(la[0] - lf[0]) + std::fabs(la[2] - lf[2]) < 0.5) la[0] += 2.0;
  const double dist = std::sqrt((lf[0] - la[0]) * (lf[0] - la[0]) + (lf[1] - la[1]) * (lf[1] - la[1]) +
                                (lf[2] - la[2]) * (lf[2] - la[2]));
  const double focus = dist * (0.3 + 1.4 * U(g));
  const double angle = kind == 0 ? 0.0 : kind == 2 ? 90.0 : 0.2 + 4.0 * U(g);   // 90 degrees: lens radius = focus distance
  float cam[18];
  int defocus;
  make_cam(w, h, 10.0 + 60.0 * U(g), lf, la, angle, focus, cam, &defocus);
  if (!defocus) ++n.no_defocus;
  if (kind == 2) ++n.wide_aperture;

  // the frame's rows as the kernel sees them (compacted row r -> image row)
  const int rows_out = step ? (h + 1) / 2 : h;
  auto image_row = [&](int r) { return step ? static_cast<float>(2 * r) : static_cast<float>(r); };
  const int tiles_x = (w + 7) / 8, tiles_y = (rows_out + th - 1) / th;

  std::vector<Body> b;
  const double wdir[3] = {(la[0] - lf[0]) / dist, (la[1] - lf[1]) / dist, (la[2] - lf[2]) / dist};
  for (int i = 0; i < 10; ++i) {   // in view, around the look direction
    const double s = dist * (0.1 + 2.0 * U(g));
    b.push_back(body(lf[0] + s * wdir[0] + sym(0.4 * s), lf[1] + s * wdir[1] + sym(0.3 * s), lf[2] + s * wdir[2] + sym(0.4 * s),
                     0.02 + 0.6 * U(g)));
  }
  for (int i = 0; i < 3; ++i) {   // behind the camera
    const double s = -dist * (0.05 + U(g));
    b.push_back(body(lf[0] + s * wdir[0] + sym(0.5), lf[1] + s * wdir[1] + sym(0.5), lf[2] + s * wdir[2] + sym(0.5), 0.05 + 0.5 * U(g)));
    ++n.behind;
  }
  for (int i = 0; i < 2; ++i) {   // around the camera: the origin inside, or on the surface
    const double r = 0.3 + 2.0 * U(g), off = i ? r * (1.0 + sym(1e-4)) : r * U(g);
    b.push_back(body(lf[0] + off * wdir[2], lf[1], lf[2] - off * wdir[0], r));
    ++n.inside;
  }
  for (int i = 0; i < 3; ++i) {   // far smaller than a pixel
    const double s = dist * (0.2 + U(g));
    b.push_back(body(lf[0] + s * wdir[0] + sym(0.1 * s), lf[1] + s * wdir[1] + sym(0.1 * s), lf[2] + s * wdir[2] + sym(0.1 * s),
                     1e-5 * std::pow(100.0, U(g))));
    ++n.tiny;
  }
  for (int i = 0; i < 2; ++i) {   // far larger: a ground, a wall
    const double r = 100.0 * std::pow(10.0, U(g));
    b.push_back(i ? body(lf[0] + (dist + r) * wdir[0], lf[1] + (dist + r) * wdir[1], lf[2] + (dist + r) * wdir[2], r * (1.0 + sym(0.5)))
                  : body(la[0], -r - 0.5 * U(g), la[2], r));
    ++n.huge;
  }
  // tangent to an extreme ray of a random tile: its centre r (1 +- eps) off a
  // point of the ray, perpendicular to it
  for (int i = 0; i < 6; ++i) {
    const int tx = static_cast<int>(U(g) * tiles_x), ty = static_cast<int>(U(g) * tiles_y);
    const int x0 = tx * 8, x1 = std::min(w, x0 + 8) - 1, r0 = ty * th, r1 = std::min(rows_out, r0 + th) - 1;
    const float px = U(g) < 0.5 ? x0 : x1, py = image_row(U(g) < 0.5 ? r0 : r1);
    const float jx = px == x0 ? -0.5f : 0.5f - 0x1p-24f, jy = U(g) < 0.5 ? -0.5f : 0.5f - 0x1p-24f;
    const double a = 6.283185307 * U(g);
    const Ray ry = camera_ray(cam, defocus, px, py, jx, jy, static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
    const double d[3] = {ry.d[0], ry.d[1], ry.d[2]};
    const double dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    // a perpendicular: d x e for a random e, normalised
    const double e[3] = {sym(1), sym(1), sym(1)};
    double p[3] = {d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]};
    const double pl = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    if (!(pl > 1e-9 * dl) || !(dl > 0)) continue;
    const double s = 0.05 + 2.5 * U(g), r = 0.01 * std::pow(100.0, U(g)), off = r * (1.0 + sym(1e-3));
    b.push_back(body(ry.o[0] + s * d[0] + off * p[0] / pl, ry.o[1] + s * d[1] + off * p[1] / pl, ry.o[2] + s * d[2] + off * p[2] / pl, r));
    ++n.tangent;
  }
  n.bodies += static_cast<long>(b.size());

  std::vector<char> keep(b.size()), keep_half(b.size());
  std::vector<float> rows;
  for (int ty = 0; ty < tiles_y; ++ty)
    for (int tx = 0; tx < tiles_x; ++tx) {
      const int x0 = tx * 8, x1 = std::min(w, x0 + 8) - 1, r0 = ty * th, r1 = std::min(rows_out, r0 + th) - 1;
      ++n.tiles;
      if (th == 1) ++n.rows1;
      if (x1 - x0 < 7 || (th == 8 && r1 - r0 < 7)) ++n.partial;
      const TileRays t = tile_rays(cam, defocus, static_cast<float>(x0), static_cast<float>(x1), image_row(r0), image_row(r1));
      const TileRays t2 = tile_rays(cam, defocus, static_cast<float>(x0), static_cast<float>(x1), image_row(r0), image_row(r1), 0.5);
      for (size_t i = 0; i < b.size(); ++i) {
        keep[i] = tile_keeps(t, b[i].c[0], b[i].c[1], b[i].c[2], b[i].w);
        keep_half[i] = tile_keeps(t2, b[i].c[0], b[i].c[1], b[i].c[2], b[i].w);
        n.kept += keep[i];
      }
      rows.clear();
      for (int r = r0; r <= r1; ++r) rows.push_back(image_row(r));
      tile_rays_each(cam, defocus, x0, x1, rows, g, [&](const Ray& ry) {
        const float len = std::sqrt(std::fmaf(ry.d[2], ry.d[2], std::fmaf(ry.d[1], ry.d[1], ry.d[0] * ry.d[0])));
        if (!(len > 0.0f)) return;
        const float il = 1.0f / len;
        const float u[3] = {ry.d[0] * il, ry.d[1] * il, ry.d[2] * il};
        ++n.rays;
        for (size_t i = 0; i < b.size(); ++i) {
          ++n.pairs;
          if (!candidate(ry, u, b[i])) continue;
          ++n.candidates;
          if (!keep[i]) {
            if (n.misses < 5)
              std::fprintf(stderr, "miss: body (%g %g %g w %g) ray o (%g %g %g) d (%g %g %g) tile x %d..%d rows %g..%g defocus %d\n",
                           b[i].c[0], b[i].c[1], b[i].c[2], b[i].w, ry.o[0], ry.o[1], ry.o[2], ry.d[0], ry.d[1], ry.d[2], x0, x1,
                           rows.front(), rows.back(), defocus);
            ++n.misses;
          }
          if (!keep_half[i]) ++n.control_misses;
        }
      });
    }
}

// C1's frame: list lengths over every tile, in bodies and in leaf records
void c1_lists(std::FILE* out) {
  const int n = rt_scene_cover(11, 42, nullptr, nullptr, nullptr, 0);
  std::vector<float> sph(4 * static_cast<size_t>(n)), mat(4 * static_cast<size_t>(n));
  std::vector<int> kind(n);
  rt_scene_cover(11, 42, sph.data(), kind.data(), mat.data(), n);
  BvhHost tree;
  bvh_build(sph.data(), n, &tree, 4, true);
  const int w = 1200, h = 675;
  const double lf[3] = {13, 2, 3}, la[3] = {0, 0, 0};
  float cam[18];
  int defocus;
  make_cam(w, h, 20.0, lf, la, 0.6, 10.0, cam, &defocus);
  const int n_rec = static_cast<int>(tree.pairs.size() / 16);
  long tiles = 0, sum_b = 0, sum_r = 0, over_b = 0, over_r = 0, empty = 0;
  int max_b = 0, max_r = 0;
  std::vector<long> hist(16, 0);   // tiles by kept bodies, 15: 15 or more (no list)
  for (int ty = 0; ty * 8 < h; ++ty)
    for (int tx = 0; tx * 8 < w; ++tx) {
      const int x0 = tx * 8, x1 = std::min(w, x0 + 8) - 1, y0 = ty * 8, y1 = std::min(h, y0 + 8) - 1;
      const TileRays t = tile_rays(cam, defocus, static_cast<float>(x0), static_cast<float>(x1), static_cast<float>(y0),
                                   static_cast<float>(y1));
      int nb = 0, nr = 0;
      for (int k = 0; k < n_rec; ++k) {
        int in_rec = 0;
        for (int j = 0; j < 4; ++j) {
          const float* p = &tree.pairs[static_cast<size_t>(2 * k + (j >> 1)) * 8];   // x0 x1 y0 y1 z0 z1 w0 w1
          in_rec += tile_keeps(t, p[j & 1], p[2 + (j & 1)], p[4 + (j & 1)], p[6 + (j & 1)]);
        }
        nb += in_rec;
        nr += in_rec > 0;
      }
      ++tiles;
      sum_b += nb, sum_r += nr;
      max_b = std::max(max_b, nb), max_r = std::max(max_r, nr);
      over_b += nb > 16, over_r += nr > 15;
      empty += nb == 0;
      ++hist[std::min(nb, 15)];
    }
  std::fprintf(out,
               "\"c1\": {\"tiles\": %ld, \"bodies\": %d, \"records\": %d, \"mean_bodies\": %.3f, \"max_bodies\": %d, "
               "\"share_over_16_bodies\": %.5f, \"mean_records\": %.3f, \"max_records\": %d, \"share_over_15_records\": %.5f, "
               "\"share_empty\": %.4f, \"tiles_by_bodies\": [",
               tiles, n, n_rec, static_cast<double>(sum_b) / tiles, max_b, static_cast<double>(over_b) / tiles,
               static_cast<double>(sum_r) / tiles, max_r, static_cast<double>(over_r) / tiles, static_cast<double>(empty) / tiles);
  for (size_t i = 0; i < hist.size(); ++i) std::fprintf(out, "%s%ld", i ? ", " : "", hist[i]);
  std::fprintf(out, "]}");
}

// `tile_list_check bodies`: tl_host_tile, the body of rt_tile_bodies_host (the
// sanitizer build lib/tile_bodies_check runs this mode).  Over random finite
// scenes, cameras and launches (partial border tiles, interleaved row tiles),
// every tile: the kept bodies are exactly those tile_keeps keeps of the
// scene's (centre, -r * r in fp32), body by body, each once; every output
// array is a heap block of exactly its size, `cap` at, below and above the
// count; a slot's entry (tl_entry over a 16-aligned record base) decodes back
// to the body's and the index's address and fits 16 bits.  One JSON line.
int bodies_mode() {
  std::mt19937 g(20241021u);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto sym = [&](double a) { return a * (2.0 * U(g) - 1.0); };
  long bad = 0, tiles = 0, kept_sum = 0, entries = 0, over14 = 0, empty = 0, stepped = 0;
  auto expect = [&](bool ok, const char* what) {
    if (!ok && bad++ < 5) std::fprintf(stderr, "tile_list_check bodies: %s\n", what);
  };
  for (int cs = 0; cs < 60; ++cs) {
    const int w = 9 + static_cast<int>(U(g) * 40), h = 5 + static_cast<int>(U(g) * 30);
    const int n = static_cast<int>(U(g) * U(g) * 90);   // 0 included
    const double lf[3] = {sym(8), sym(3) + 1.0, 6.0 + sym(2)}, la[3] = {sym(1), sym(1), sym(1)};
    float cam[18];
    int defocus;
    make_cam(w, h, 15.0 + 50.0 * U(g), lf, la, cs % 3 ? 0.5 + 3.0 * U(g) : 0.0, 6.0, cam, &defocus);
    std::vector<float> sph(4 * static_cast<size_t>(std::max(n, 1)));
    for (int i = 0; i < n; ++i) {
      const bool twin = i > 0 && U(g) < 0.1;   // coincident bodies: each is listed
      for (int k = 0; k < 3; ++k) sph[4 * i + k] = twin ? sph[4 * (i - 1) + k] : static_cast<float>(sym(k == 1 ? 1.5 : 4.0));
      sph[4 * i + 3] = twin ? sph[4 * (i - 1) + 3] : static_cast<float>(U(g) < 0.05 ? 50.0 + 500.0 * U(g) : 0.02 + 0.7 * U(g));
    }
    TlFrame f{w, h, 0, 8, 0, 0};
    if (cs % 4 == 3) {   // the odd row tiles of height T from row_begin
      const int T = cs % 8 == 3 ? 1 : 8, rb = static_cast<int>(U(g) * 3), span = h - rb, nt = (span + T - 1) / T;
      int rows = 0;
      for (int t = 1; t < nt; t += 2) rows += std::min(T, span - t * T);
      f = TlFrame{w, rows, rb, T, 1, 2};
      ++stepped;
    }
    const int n_tiles = ((w + 7) / 8) * ((f.rows_out + 7) / 8);
    for (int tile = 0; tile <= n_tiles; ++tile) {   // (one past the frame: no pixels, 0)
      float x0, x1, y0, y1;
      const bool has = tl_rect(f, 8, tile, &x0, &x1, &y0, &y1);
      std::vector<int> want;
      if (has) {
        const TileRays t = tile_rays(cam, defocus, x0, x1, y0, y1);
        for (int i = 0; i < n; ++i) {
          const float r = sph[4 * i + 3];
          if (tile_keeps(t, sph[4 * i], sph[4 * i + 1], sph[4 * i + 2], -(r * r))) want.push_back(i);
        }
      }
      const int cnt = static_cast<int>(want.size());
      for (int cap : {cnt, cnt > 0 ? cnt - 1 : 0, cnt + 3}) {
        std::unique_ptr<int[]> bodies(new int[cap]), slots(new int[cap]);
        for (int i = 0; i < cap; ++i) bodies[i] = slots[i] = -7;
        const int got = tl_host_tile(sph.data(), n, true, cam, defocus, f, tile, bodies.get(), slots.get(), cap);
        expect(got == cnt, "the count differs from tile_keeps body by body");
        std::vector<int> have(bodies.get(), bodies.get() + std::min(cap, cnt));
        for (int i = std::min(cap, cnt); i < cap; ++i) expect(bodies[i] == -7 && slots[i] == -7, "written past the count");
        if (cap >= cnt) {
          std::sort(have.begin(), have.end());
          expect(have == want, "the kept bodies differ from tile_keeps body by body");
          for (int i = 0; i < cnt; ++i) {
            const unsigned base = 16u * static_cast<unsigned>(U(g) * 200), rec = base + kTlRecBytes * static_cast<unsigned>(slots[i] >> 2);
            const unsigned j = static_cast<unsigned>(slots[i] & 3), e = tl_entry(rec, j);
            expect(slots[i] >= 0 && e <= 0xffffu, "a slot outside the records, or an entry above 16 bits");
            expect(tl_body_addr(e) == rec + 16u * j && tl_index_addr(e) == rec + 64u + 4u * j, "an entry decodes to another address");
            ++entries;
          }
        }
      }
      ++tiles;
      kept_sum += cnt;
      over14 += cnt > kTlMax;
      empty += cnt == 0;
    }
  }
  std::printf("{\"tiles\": %ld, \"kept\": %ld, \"entries\": %ld, \"tiles_over_14\": %ld, \"tiles_empty\": %ld, "
              "\"interleaved_cases\": %ld, \"bad\": %ld}\n", tiles, kept_sum, entries, over14, empty, stepped, bad);
  return bad == 0 && over14 > 0 && empty > 0 && stepped > 0 ? 0 : 1;
}

// `tile_list_check count FILE`: the list length of one pixel rectangle of a
// scene given as text -- 18 camera floats (center, p00, du, dv, disk_u,
// disk_v) and the defocus flag; x0 x1 y0 y1 (first and last pixel centres:
// columns, image rows); then cx cy cz r per body -- as the kernel's prologue
// counts it: tile_keeps over every body's (centre, -r * r in fp32).  Prints
// the count (tests/test_gpu_prelude.py builds tiles of 15, 16 and 17 with it).
int count_file(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) {
    std::fprintf(stderr, "tile_list_check: cannot read %s\n", path);
    return 2;
  }
  float cam[18], r4[4];
  int defocus = 0;
  for (float& c : cam)
    if (std::fscanf(f, "%f", &c) != 1) return 2;
  if (std::fscanf(f, "%d", &defocus) != 1) return 2;
  for (float& c : r4)
    if (std::fscanf(f, "%f", &c) != 1) return 2;
  const TileRays t = tile_rays(cam, defocus, r4[0], r4[1], r4[2], r4[3]);
  float b[4];
  int kept = 0, n = 0;
  while (std::fscanf(f, "%f %f %f %f", &b[0], &b[1], &b[2], &b[3]) == 4) {
    kept += tile_keeps(t, b[0], b[1], b[2], -(b[3] * b[3]));
    ++n;
  }
  std::fclose(f);
  std::printf("{\"bodies\": %d, \"kept\": %d}\n", n, kept);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 2 && std::string(argv[1]) == "count") return count_file(argv[2]);
  if (argc > 1 && std::string(argv[1]) == "bodies") return bodies_mode();
  const long want = argc > 1 ? std::atol(argv[1]) : 5000000;   // candidate pairs at least
  std::mt19937 g(20240611u);
  Counts n;
  long cases = 0;
  while (n.candidates < want) {
    run_case(g, n);
    ++cases;
  }
  std::printf("{\"cases\": %ld, \"tiles\": %ld, \"rays\": %ld, \"pairs\": %ld, \"candidates\": %ld, \"misses\": %ld, "
              "\"control_misses\": %ld, \"kept_share\": %.4f, \"no_defocus\": %ld, \"wide_aperture\": %ld, \"inside\": %ld, "
              "\"behind\": %ld, \"tangent\": %ld, \"tiny\": %ld, \"huge\": %ld, \"one_row_tiles\": %ld, \"partial_tiles\": %ld, ",
              cases, n.tiles, n.rays, n.pairs, n.candidates, n.misses, n.control_misses,
              static_cast<double>(n.kept) / (static_cast<double>(n.bodies) / cases * n.tiles), n.no_defocus, n.wide_aperture, n.inside,
              n.behind, n.tangent, n.tiny, n.huge, n.rows1, n.partial);
  c1_lists(stdout);
  std::printf("}\n");
  return n.misses == 0 && n.control_misses > 0 ? 0 : 1;
}
