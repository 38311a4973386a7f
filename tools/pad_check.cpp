// pad_check.cpp — CPU property check of the BVH walk's box padding, on the
// text the kernel runs (raytracing-clj_amd/csrc/bvh_pad.h, host build).
//
// For random and directed (body, ray) cases it runs the scan's fp32 body test
// (trace_kernel.h's op sequence, self-hit guard included).  For every
// candidate the test accepts with root t, the body's own box and every box of
// a chain of random unions around it (its ancestors in a small random tree,
// stored as bvh.cpp stores them: relative to the tree centre, rounded
// outward) must pass the walk's slab test with best_t = t:
//     tn <= min(tf, t)  and  tmin <= tf.
// A box that fails is a false cull: the walk would have missed a hit the scan
// reports.  Prints one JSON line; exit status 1 on any false cull.
//
// Random cases: tools/pad_bound.cpp's generator (both origin scales), one in
// eight with the origin on the body the ray leaves (sq = |h|).  Directed
// cases (counted apart): direction components around the per-axis limit and
// around k, exact zeros, tangency from ~1000 units, r = 1e-3 bodies (the
// rounding term), an r = 5 body among r = 0.05 ones, origins inside boxes,
// short chords (2 h around tmin) out of small bodies.
//
// g++ -O2 -std=c++17 -ffp-contract=off -mfma tools/pad_check.cpp -o pad_check && ./pad_check [trials]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../raytracing-clj_amd/csrc/bvh_pad.h"

using namespace rtclj;

namespace {

struct Sph {
  float c[3], r;
};
struct Counts {
  long cases = 0, accepted = 0, boxes = 0, false_culls = 0, all_new = 0, any_axis_old = 0, ray_old = 0, self_hit = 0;
};

// one case: body b[0] is the one tested, b[1..] its companions in the tree
void check(const std::vector<Sph>& b, const float o[3], const float d[3], bool self, Counts& n) {
  ++n.cases;
  const float len = std::sqrt(std::fmaf(d[2], d[2], std::fmaf(d[1], d[1], d[0] * d[0])));
  if (!(len > 0.0f)) return;
  const float il = 1.0f / len;
  const float u[3] = {d[0] * il, d[1] * il, d[2] * il};
  const float tmin = 1e-3f * len;
  // the scan's test of body 0
  const Sph& s = b[0];
  const float nr2 = -(s.r * s.r);
  const float ocx = s.c[0] - o[0], ocy = s.c[1] - o[1], ocz = s.c[2] - o[2];
  const float h = std::fmaf(u[2], ocz, std::fmaf(u[1], ocy, u[0] * ocx));
  const float c = std::fmaf(ocx, ocx, std::fmaf(ocz, ocz, std::fmaf(ocy, ocy, nr2)));
  const float disc = std::fmaf(h, h, -c);
  if (!(disc >= 0.0f) || (h < 0.0f && c >= 0.0f)) return;   // the leaf pass' candidate test
  const float sq = self ? std::fabs(h) : std::sqrt(disc);
  const float t0 = h - sq;
  const float t = t0 > tmin ? t0 : h + sq;
  if (!(t > tmin)) return;
  ++n.accepted;
  if (self) ++n.self_hit;
  // the tree's bounding sphere and r_max, as bvh.cpp
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (const Sph& q : b)
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], double(std::nextafter(q.c[k] - q.r, -INFINITY)));
      hi[k] = std::max(hi[k], double(std::nextafter(q.c[k] + q.r, INFINITY)));
    }
  double bc[3], br = 0, rmax = 0;
  for (int k = 0; k < 3; ++k) bc[k] = 0.5 * (lo[k] + hi[k]);
  for (const Sph& q : b) {
    const double dx = q.c[0] - bc[0], dy = q.c[1] - bc[1], dz = q.c[2] - bc[2];
    br = std::max(br, std::sqrt(dx * dx + dy * dy + dz * dz) + q.r);
    rmax = std::max(rmax, double(q.r));
  }
  const float cf[3] = {float(bc[0]), float(bc[1]), float(bc[2])};
  const float R = float(br * (1.0 + 1e-6)) + 1e-6f;
  const float c0 = kPadRmax * float(rmax * (1.0 + 1e-6));
  // the walk's set-up
  const float e[3] = {o[0] - cf[0], o[1] - cf[1], o[2] - cf[2]};
  const PadRay pr = pad_ray(e[0], e[1], e[2], u[0], u[1], u[2], R, c0);
  const PadAxis ax[3] = {pad_axis(u[0], e[0], tmin, pr), pad_axis(u[1], e[1], tmin, pr), pad_axis(u[2], e[2], tmin, pr)};
  // the form the ray took, and why not the per-distance one
  const float umin = std::fmin(std::fmin(std::fabs(u[0]), std::fabs(u[1])), std::fabs(u[2]));
  if (pr.per_t) ++n.all_new;
  else if (!(umin > kPadLimit)) ++n.any_axis_old;
  else ++n.ray_old;
  // the body's box, then the unions with its companions one by one
  float blo[3], bhi[3];
  for (int k = 0; k < 3; ++k) {
    blo[k] = std::nextafter(s.c[k] - s.r, -INFINITY);
    bhi[k] = std::nextafter(s.c[k] + s.r, INFINITY);
  }
  for (size_t j = 0; j < b.size(); ++j) {
    if (j > 0)
      for (int k = 0; k < 3; ++k) {
        blo[k] = std::min(blo[k], std::nextafter(b[j].c[k] - b[j].r, -INFINITY));
        bhi[k] = std::max(bhi[k], std::nextafter(b[j].c[k] + b[j].r, INFINITY));
      }
    float pn[3], pf[3];
    for (int k = 0; k < 3; ++k) {
      const float l = std::nextafter(float(double(blo[k]) - cf[k]), -INFINITY);
      const float g = std::nextafter(float(double(bhi[k]) - cf[k]), INFINITY);
      pn[k] = ax[k].sign ? g : l;
      pf[k] = ax[k].sign ? l : g;
    }
    float tn, tf;
    pad_interval(ax[0], ax[1], ax[2], pn[0], pf[0], pn[1], pf[1], pn[2], pf[2], tn, tf);
    ++n.boxes;
    if (!pad_meets(tn, tf, tmin, t)) {
      if (++n.false_culls <= 5)
        std::fprintf(stderr, "false cull: box %zu o=(%.9g %.9g %.9g) u=(%.9g %.9g %.9g) body=(%.9g %.9g %.9g r %.9g) t=%.9g tn=%.9g tf=%.9g\n",
                     j, o[0], o[1], o[2], u[0], u[1], u[2], s.c[0], s.c[1], s.c[2], s.r, t, tn, tf);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  const long trials = argc > 1 ? std::atol(argv[1]) : 2000000;
  std::mt19937_64 g(12345);
  std::uniform_real_distribution<double> U(-1, 1);
  auto body = [&](double rlo, double rhi) {
    Sph s;
    s.c[0] = float(U(g) * 30);
    s.c[1] = float(U(g) * 3);
    s.c[2] = float(U(g) * 30);
    s.r = float(std::exp(std::log(rlo) + (U(g) * 0.5 + 0.5) * std::log(rhi / rlo)));
    return s;
  };
  auto companions = [&](std::vector<Sph>& b, double rlo, double rhi) {
    const int m = 1 + int((U(g) * 0.5 + 0.5) * 5.999);
    for (int i = 0; i < m; ++i) b.push_back(body(rlo, rhi));
  };
  // a direction from o at the body's silhouette region (pad_bound.cpp's aim)
  auto aim = [&](const Sph& s, const float o[3], float d[3]) {
    for (int k = 0; k < 3; ++k) d[k] = float(double(s.c[k]) - o[k] + U(g) * s.r * 1.2);
  };
  // an origin on body s as the kernel makes one: the fp32 hit point of an
  // earlier ray (p = o + t u, one fma per component); false if that ray missed
  auto surface_origin = [&](const Sph& s, float o[3]) {
    // (one in five from ~1000 units: the hit point is then off the surface by
    // up to 6e-4 * 1000, far more than the padding at the next segment's t)
    const double S0 = U(g) > 0.6 ? 1000.0 : 30.0;
    float o0[3] = {float(U(g) * S0), float(U(g) * S0 * 0.1 + 1), float(U(g) * S0)}, d[3];
    for (int k = 0; k < 3; ++k) d[k] = float(double(s.c[k]) - o0[k] + U(g) * s.r * 0.9);
    const float len = std::sqrt(std::fmaf(d[2], d[2], std::fmaf(d[1], d[1], d[0] * d[0])));
    const float u[3] = {d[0] / len, d[1] / len, d[2] / len};
    const float ocx = s.c[0] - o0[0], ocy = s.c[1] - o0[1], ocz = s.c[2] - o0[2];
    const float h = std::fmaf(u[2], ocz, std::fmaf(u[1], ocy, u[0] * ocx));
    const float c = std::fmaf(ocx, ocx, std::fmaf(ocz, ocz, std::fmaf(ocy, ocy, -(s.r * s.r))));
    const float disc = std::fmaf(h, h, -c);
    if (!(disc >= 0.0f)) return false;
    const float t = h - std::sqrt(disc);
    if (!(t > 1e-3f * len)) return false;
    for (int k = 0; k < 3; ++k) o[k] = std::fmaf(t, u[k], o0[k]);
    return true;
  };

  Counts rnd, dir;
  for (long it = 0; it < trials; ++it) {
    const double S = (it % 10 == 0) ? 1000.0 : 30.0;
    std::vector<Sph> b{body(0.05, 2.0)};
    companions(b, 0.05, 2.0);
    float o[3], d[3];
    if (it % 8 == 7) {
      // the ray leaves body 0: a direction into it (t = 2 h needs h > 0)
      if (!surface_origin(b[0], o)) continue;
      for (int k = 0; k < 3; ++k) d[k] = float(U(g));
      const double dot = double(d[0]) * (b[0].c[0] - o[0]) + double(d[1]) * (b[0].c[1] - o[1]) + double(d[2]) * (b[0].c[2] - o[2]);
      if (dot < 0)
        for (int k = 0; k < 3; ++k) d[k] = -d[k];
      check(b, o, d, true, rnd);
      continue;
    }
    o[0] = float(U(g) * S);
    o[1] = float(U(g) * S * 0.1 + 1);
    o[2] = float(U(g) * S);
    aim(b[0], o, d);
    check(b, o, d, false, rnd);
  }

  // ---- directed cases ----
  const long nd = std::max(1000L, trials / 40);
  // 1) near-axis rays: the main component along +-axis a, the others at
  // f * k for f around the limit (1.5), around 1 and at exact zero
  const double fs[] = {0.0, 0.5, 0.9, 0.99, 1.0, 1.01, 1.4, 1.49, 1.5, 1.51, 1.6, 2.0, 3.0};
  for (long it = 0; it < nd; ++it) {
    std::vector<Sph> b{body(0.05, 2.0)};
    companions(b, 0.05, 2.0);
    const int a = int(it % 3), sg = (it / 3) % 2 ? -1 : 1;
    const double L = (it % 5 == 0) ? 1000.0 : 5.0 + 20.0 * (U(g) * 0.5 + 0.5);
    double dd[3];
    dd[a] = sg;
    const double f1 = fs[(it / 6) % 13], f2 = fs[(it / 78) % 13];
    dd[(a + 1) % 3] = ((it / 7) % 2 ? -1 : 1) * f1 * double(kPadK);
    dd[(a + 2) % 3] = ((it / 11) % 2 ? -1 : 1) * f2 * double(kPadK);
    // the origin L back along dd from a point inside the body, so the ray hits
    float o[3], d[3];
    double p[3];
    for (int k = 0; k < 3; ++k) p[k] = b[0].c[k] + U(g) * b[0].r * 0.55;
    for (int k = 0; k < 3; ++k) o[k] = float(p[k] - L * dd[k]);
    for (int k = 0; k < 3; ++k) d[k] = float(dd[k] * L);
    if (f1 == 0.0) d[(a + 1) % 3] = (it / 7) % 2 ? -0.0f : 0.0f;
    if (f2 == 0.0) d[(a + 2) % 3] = (it / 11) % 2 ? -0.0f : 0.0f;
    check(b, o, d, false, dir);
  }
  // 2) tangency from far away: a row of equal small spheres seen edge-on
  for (long it = 0; it < nd; ++it) {
    std::vector<Sph> b;
    const float r = 0.2f;
    const int m = 2 + int(it % 6);
    for (int i = 0; i < m; ++i) b.push_back(Sph{{float(i) * 0.5f, 0.0f, 0.0f}, r});
    std::swap(b[0], b[it % m]);
    float o[3] = {float(-1000.0 + U(g) * 50), float(U(g) * 0.01), float(U(g) * 0.01)}, d[3];
    // aimed at the rim: offset r * (1 + tiny) perpendicular to the row
    const double ang = U(g) * 3.14159265358979, rim = r * (1.0 + U(g) * 2e-3);
    d[0] = float(b[0].c[0] - o[0]);
    d[1] = float(rim * std::cos(ang) - o[1]);
    d[2] = float(rim * std::sin(ang) - o[2]);
    check(b, o, d, false, dir);
  }
  // 3) tiny bodies (the rounding term decides), near and far origins
  for (long it = 0; it < nd; ++it) {
    std::vector<Sph> b{body(1e-3, 1.001e-3)};
    companions(b, 1e-3, 1.001e-3);
    const double S = (it % 3 == 0) ? 1000.0 : 30.0;
    float o[3] = {float(U(g) * S), float(U(g) * S * 0.1 + 1), float(U(g) * S)}, d[3];
    aim(b[0], o, d);
    check(b, o, d, false, dir);
  }
  // 4) one r = 5 body among r = 0.05 ones (either one as the body tested)
  for (long it = 0; it < nd; ++it) {
    std::vector<Sph> b{body(0.05, 0.0501)};
    companions(b, 0.05, 0.0501);
    Sph big = body(5.0, 5.001);
    if (it % 2) b.push_back(big);
    else b.insert(b.begin(), big);
    const double S = (it % 4 == 0) ? 1000.0 : 30.0;
    float o[3] = {float(U(g) * S), float(U(g) * S * 0.1 + 1), float(U(g) * S)}, d[3];
    // (one in four a compact tree around the big body, seen from close by:
    // D < 3 r_max, the ray-wide fallback)
    if (it % 4 == 1) {
      for (Sph& q : b)
        if (q.r < 1.0f)
          for (int k = 0; k < 3; ++k) q.c[k] = float(big.c[k] + U(g) * 6.0);
      for (int k = 0; k < 3; ++k) o[k] = float(big.c[k] + U(g) * 7.0);
    }
    aim(b[0], o, d);
    check(b, o, d, false, dir);
  }
  // 5) origins inside boxes: inside the body (glass: the far root), on its
  // surface leaving through it, and on a touching neighbour's surface
  for (long it = 0; it < nd; ++it) {
    std::vector<Sph> b{body(0.05, 2.0)};
    Sph touch = b[0];
    touch.c[0] += 2.0f * b[0].r;   // touching sphere
    b.push_back(touch);
    companions(b, 0.05, 2.0);
    float o[3], d[3];
    const int mode = int(it % 3);
    if (mode == 0) {
      for (int k = 0; k < 3; ++k) o[k] = float(b[0].c[k] + U(g) * b[0].r * 0.57);
      for (int k = 0; k < 3; ++k) d[k] = float(U(g));
      check(b, o, d, false, dir);
    } else if (mode == 1) {
      if (!surface_origin(b[0], o)) continue;
      for (int k = 0; k < 3; ++k) d[k] = float(b[0].c[k] - o[k] + U(g) * b[0].r);
      check(b, o, d, true, dir);
    } else {
      if (!surface_origin(b[1], o)) continue;
      aim(b[0], o, d);
      check(b, o, d, false, dir);
    }
  }

  // 6) leaving a small body along a short chord: r a few times tmin, so the
  // guard's root 2 h lies just above tmin and the chord's midpoint below it
  for (long it = 0; it < nd; ++it) {
    std::vector<Sph> b{body(1e-3, 2e-2)};
    companions(b, 1e-3, 2e-2);
    float o[3], d[3];
    if (!surface_origin(b[0], o)) continue;
    // a unit direction with h = u . oc in (0.4, 1.2) x 1e-3: 2 h around tmin
    double oc[3], n2 = 0, w[3], wn = 0;
    for (int k = 0; k < 3; ++k) oc[k] = double(b[0].c[k]) - o[k], n2 += oc[k] * oc[k];
    const double rho = std::sqrt(n2), hh = (0.4 + 0.8 * (U(g) * 0.5 + 0.5)) * 1e-3;
    for (int k = 0; k < 3; ++k) w[k] = U(g);
    double dot = 0;
    for (int k = 0; k < 3; ++k) dot += w[k] * oc[k] / rho;
    for (int k = 0; k < 3; ++k) w[k] -= dot * oc[k] / rho, wn += w[k] * w[k];
    wn = std::sqrt(wn);
    const double ca = std::min(1.0, hh / rho), sa = std::sqrt(1.0 - ca * ca);
    for (int k = 0; k < 3; ++k) d[k] = float(ca * oc[k] / rho + sa * w[k] / wn);
    check(b, o, d, true, dir);
  }

  auto line = [](const char* name, const Counts& n) {
    std::printf("\"%s\": {\"cases\": %ld, \"accepted\": %ld, \"boxes\": %ld, \"false_culls\": %ld, \"all_axes_per_distance\": %ld, "
                "\"some_axis_ray_wide\": %ld, \"ray_fallback\": %ld, \"self_hit\": %ld}",
                name, n.cases, n.accepted, n.boxes, n.false_culls, n.all_new, n.any_axis_old, n.ray_old, n.self_hit);
  };
  std::printf("{");
  line("random", rnd);
  std::printf(", ");
  line("directed", dir);
  std::printf("}\n");
  return rnd.false_culls + dir.false_culls ? 1 : 0;
}
