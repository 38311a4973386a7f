// rays_check — the ray queries' host side (csrc/ray_query.h: rays_host_pass and
// occluded_host_pass, the bodies of rt_rays_host and rt_occluded_host, with the
// set-up, the search and the record the kernels run) built for the host under
// the sanitizers.  A program of its own: never loaded into another process.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all -static-libasan -static-libubsan tools/rays_check.cpp csrc/bvh.cpp csrc/scenes.cpp
//
//   rays_check
// Every array is a heap block of exactly its size.  Scenes with NaN, infinite,
// zero, negative and 3e38 centres and radii; rays whose every field may be one
// of those too; `last` far out of range, INT32_MIN and INT32_MAX among them;
// valid rays, every inactive class of rt.h's step 2, rays that leave a surface
// with and without the guard; n = 0 with NULL arrays; NULL arguments.  Exit
// status 0 when every call returned what it should, every body lies in
// [-1, n), every inactive ray has the "none" record and every occlusion byte
// equals body >= 0.
//
//   rays_check walk N SEED [--scene FILE]
// The walk against the scan on query rays -- not the renderer's: origins far
// outside the tree, deep inside bodies and on surfaces, t_min 0 or small,
// t_max finite for half of them, |d| from 2^-6 to 2^6, a guarded body for a
// third.  Per ray and for each of bvh_build's three trees, fh_walk<true> must
// give fh_scan<true>'s (body, t bits) from {t_max |d|, -1}, and fh_walk_any
// must give body >= 0.  N rays on each of the reference scene, rt_scene_cover's
// 484 and 1025 bodies, or on FILE's bodies (raw little-endian float32, n x
// (cx, cy, cz, r)).  One JSON line; exit status 1 on a mismatch.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../include/rt.h"
#include "../raytracing-clj_amd/csrc/bvh.h"
#include "../raytracing-clj_amd/csrc/ray_query.h"

using namespace rtclj;

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double unit() { return static_cast<double>(next() >> 11) * 0x1p-53; }
  double sym() { return 2.0 * unit() - 1.0; }
  float uni() { return static_cast<float>(next() >> 40) * 0x1p-24f; }
};

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

template <class T>
std::unique_ptr<T[]> block(size_t n) {
  return std::unique_ptr<T[]>(new T[n]);
}

// ------------------------------------------------- the sanitizer run ----
const float kOdd[] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, -1.0f, -4.0f, 1e-42f, 3e38f, -3e38f, 0x1p40f, -0x1p40f};
const int32_t kOddId[] = {INT32_MIN, INT32_MAX, -1, -2, 1 << 30, -(1 << 30), 65536, 0x7ffffff0};

float draw(Rng& r, float lo, float hi, float p) {
  if (r.uni() < p) return kOdd[r.next() % (sizeof kOdd / sizeof kOdd[0])];
  return lo + (hi - lo) * r.uni();
}

struct Scene {
  int n;
  std::unique_ptr<float[]> sphere;
  rt_scene c;
};
Scene scene(Rng& rng, int n, float p_odd) {
  Scene s{n, block<float>(4 * static_cast<size_t>(n)), rt_scene{}};
  for (int b = 0; b < n; ++b) {
    for (int c = 0; c < 2; ++c) s.sphere[4 * b + c] = draw(rng, -1.5f, 1.5f, p_odd);
    s.sphere[4 * b + 2] = draw(rng, -8.0f, -2.0f, p_odd);
    s.sphere[4 * b + 3] = draw(rng, 0.05f, 0.6f, p_odd);
  }
  s.c.n = n;
  s.c.sphere = n ? s.sphere.get() : nullptr;   // (the queries read no material)
  return s;
}

bool is_none(const rt_ray_hit& h) {
  return h.body == -1 && h.front_face == 0 && bits(h.t) == 0x7f800000u && bits(h.dist) == 0x7f800000u &&
         bits(h.normal[0]) == 0 && bits(h.normal[1]) == 0 && bits(h.normal[2]) == 0 && bits(h.reserved) == 0;
}

rt_ray make_ray(float ox, float oy, float oz, float t_min, float dx, float dy, float dz, float t_max) {
  rt_ray r;
  r.o[0] = ox, r.o[1] = oy, r.o[2] = oz, r.t_min = t_min;
  r.d[0] = dx, r.d[1] = dy, r.d[2] = dz, r.t_max = t_max;
  return r;
}

int sanitizer_run() {
  Rng rng{97531};
  long calls = 0, rays_all = 0, hits = 0, inactive = 0, bad = 0;
  const char* why = nullptr;
  // 1) random and hostile scenes, rays and `last`
  const int counts[] = {0, 1, 5, 64, 65, 300};
  for (int n : counts)
    for (float p_scene : {0.0f, 0.3f})
      for (float p_ray : {0.0f, 0.25f}) {
        Scene sc = scene(rng, n, p_scene);
        const size_t m = 257;
        auto rays = block<rt_ray>(m);
        auto last = block<int32_t>(m);
        auto out = block<rt_ray_hit>(m);
        auto occ = block<uint8_t>(m);
        for (size_t i = 0; i < m; ++i) {
          rays[i] = make_ray(draw(rng, -1.0f, 1.0f, p_ray), draw(rng, -1.0f, 1.0f, p_ray), draw(rng, -1.0f, 1.0f, p_ray),
                             draw(rng, 0.0f, 0.01f, p_ray), draw(rng, -0.3f, 0.3f, p_ray), draw(rng, -0.3f, 0.3f, p_ray),
                             draw(rng, -2.0f, -0.5f, p_ray), rng.uni() < 0.5f ? INFINITY : draw(rng, 0.5f, 8.0f, p_ray));
          last[i] = rng.uni() < 0.3f ? kOddId[rng.next() % (sizeof kOddId / sizeof kOddId[0])]
                                     : static_cast<int32_t>(rng.next() % static_cast<uint64_t>(n + 2)) - 1;
        }
        for (int with_last = 0; with_last < 2; ++with_last) {
          const int32_t* lp = with_last ? last.get() : nullptr;
          bad += rays_host_pass(&sc.c, rays.get(), lp, m, out.get(), &why) != RT_OK;
          bad += occluded_host_pass(&sc.c, rays.get(), lp, m, occ.get(), &why) != RT_OK;
          calls += 2;
          for (size_t i = 0; i < m; ++i) {
            const rt_ray_hit& h = out[i];
            ++rays_all;
            bad += h.body < -1 || h.body >= n;
            bad += occ[i] != (h.body >= 0 ? 1 : 0);
            if (h.body < 0) {
              bad += !is_none(h);
            } else {
              ++hits;
              bad += !(h.dist > 0.0f) || !(h.t > 0.0f) || (h.front_face != 0 && h.front_face != 1) ||
                     bits(h.reserved) != 0 || h.normal[0] != h.normal[0] || h.normal[1] != h.normal[1] ||
                     h.normal[2] != h.normal[2];
              bad += !(h.t <= rays[i].t_max * 1.001f) || !(h.t >= rays[i].t_min * 0.999f);
            }
          }
        }
      }
  // 2) the inactive classes of rt.h's step 2, one by one, on a scene each would hit
  {
    auto sph = block<float>(4);
    sph[0] = 0.0f, sph[1] = 0.0f, sph[2] = -3.0f, sph[3] = 1.0f;
    rt_scene sc{};
    sc.n = 1;
    sc.sphere = sph.get();
    const rt_ray cls[] = {
        make_ray(NAN, 0, 0, 0, 0, 0, -1, INFINITY),        make_ray(0, INFINITY, 0, 0, 0, 0, -1, INFINITY),
        make_ray(0, 0, -INFINITY, 0, 0, 0, -1, INFINITY),  make_ray(0, 0, 0, 0, 0, 0, 0, INFINITY),
        make_ray(0, 0, 0, 0, 0, 0, -0.0f, INFINITY),       make_ray(0, 0, 0, 0, 1e-30f, 0, -1e-30f, INFINITY),
        make_ray(0, 0, 0, 0, 0, NAN, -1, INFINITY),        make_ray(0, 0, 0, 0, 0, 0, -INFINITY, INFINITY),
        make_ray(0, 0, 0, 0, 0, 0, -3e19f, INFINITY),      make_ray(0, 0, 0, NAN, 0, 0, -1, INFINITY),
        make_ray(0, 0, 0, -1e-3f, 0, 0, -1, INFINITY),     make_ray(0, 0, 0, 0, 0, 0, -1, NAN),
        make_ray(0, 0, 0, 1.0f, 0, 0, -1, 1.0f),           make_ray(0, 0, 0, 2.5f, 0, 0, -1, 2.25f),
        make_ray(0, 0, 0, INFINITY, 0, 0, -1, INFINITY),   make_ray(0, 0, 0, 0, 0, 0, -1, 0),
        make_ray(0, 0, 0, 0, 0, 0, -1, -1.0f),
    };
    const size_t m = sizeof cls / sizeof cls[0];
    auto rays = block<rt_ray>(m + 1);
    for (size_t i = 0; i < m; ++i) rays[i] = cls[i];
    rays[m] = make_ray(0, 0, 0, 0, 0, 0, -1, INFINITY);   // the valid one: hit at t = 2
    auto out = block<rt_ray_hit>(m + 1);
    auto occ = block<uint8_t>(m + 1);
    bad += rays_host_pass(&sc, rays.get(), nullptr, m + 1, out.get(), &why) != RT_OK;
    bad += occluded_host_pass(&sc, rays.get(), nullptr, m + 1, occ.get(), &why) != RT_OK;
    calls += 2;
    for (size_t i = 0; i < m; ++i) {
      bad += !is_none(out[i]) || occ[i] != 0;
      ++inactive;
    }
    const rt_ray_hit& h = out[m];
    bad += h.body != 0 || h.front_face != 1 || h.t != 2.0f || h.dist != 2.0f || h.normal[2] != 1.0f || occ[m] != 1;
    // a strict upper bound: t_max = 2 misses the hit at 2, the next float up does not
    rays[0] = make_ray(0, 0, 0, 0, 0, 0, -1, 2.0f);
    rays[1] = make_ray(0, 0, 0, 0, 0, 0, -1, std::nextafter(2.0f, 3.0f));
    // in |d| units: d twice as long, the hit at t = 1, dist = 2
    rays[2] = make_ray(0, 0, 0, 0, 0, 0, -2, INFINITY);
    // from inside the body: the far root, a back face, the normal against d
    rays[3] = make_ray(0, 0, -3, 0, 0, 0, -1, INFINITY);
    bad += rays_host_pass(&sc, rays.get(), nullptr, 4, out.get(), &why) != RT_OK;
    ++calls;
    bad += !is_none(out[0]) || out[1].body != 0 || out[2].t != 1.0f || out[2].dist != 2.0f;
    bad += out[3].body != 0 || out[3].front_face != 0 || out[3].dist != 1.0f || out[3].normal[2] != 1.0f;
  }
  // 3) a ray that leaves a surface: unguarded it meets its own body at about 0,
  //    guarded at the chord's end (inward) or not at all (outward)
  long guarded = 0;
  {
    auto sph = block<float>(8);
    const float body[8] = {0.3f, -0.2f, -3.0f, 0.7f, 5.0f, 0.0f, -3.0f, 0.5f};
    std::memcpy(sph.get(), body, sizeof body);
    rt_scene sc{};
    sc.n = 2;
    sc.sphere = sph.get();
    const size_t m = 64;
    auto rays = block<rt_ray>(2 * m);
    auto last = block<int32_t>(2 * m);
    auto out = block<rt_ray_hit>(2 * m);
    auto out0 = block<rt_ray_hit>(2 * m);
    for (size_t i = 0; i < m; ++i) {
      double v[3], l2;
      do {
        l2 = 0;
        for (int k = 0; k < 3; ++k) v[k] = rng.sym(), l2 += v[k] * v[k];
      } while (l2 > 1.0 || l2 < 1e-3);
      const double il = 1.0 / std::sqrt(l2);
      float p[3], nrm[3];
      for (int k = 0; k < 3; ++k) {
        nrm[k] = static_cast<float>(v[k] * il);
        p[k] = static_cast<float>(body[k] + 0.7 * v[k] * il);
      }
      // inward along -n with a tilt, outward along +n
      rays[2 * i] = make_ray(p[0], p[1], p[2], 0, -nrm[0] + 0.2f * nrm[1], -nrm[1] + 0.2f * nrm[2], -nrm[2] + 0.2f * nrm[0],
                             INFINITY);
      rays[2 * i + 1] = make_ray(p[0], p[1], p[2], 0, nrm[0], nrm[1], nrm[2], INFINITY);
      last[2 * i] = last[2 * i + 1] = 0;
    }
    bad += rays_host_pass(&sc, rays.get(), last.get(), 2 * m, out.get(), &why) != RT_OK;
    bad += rays_host_pass(&sc, rays.get(), nullptr, 2 * m, out0.get(), &why) != RT_OK;
    calls += 2;
    for (size_t i = 0; i < m; ++i) {
      const rt_ray_hit &in = out[2 * i], &outw = out[2 * i + 1];
      bad += in.body != 0 || !(in.dist > 0.5f) || in.front_face != 0;   // the chord: well inside 1.4
      bad += outw.body == 0;
      guarded += in.body == 0;
      // unguarded, the inward ray meets the body within the surface's rounding or at the chord's end
      bad += out0[2 * i].body != 0;
    }
    // last >= n names no body: the unguarded records
    for (size_t i = 0; i < 2 * m; ++i) last[i] = 2 + static_cast<int32_t>(i);
    bad += rays_host_pass(&sc, rays.get(), last.get(), 2 * m, out.get(), &why) != RT_OK;
    ++calls;
    bad += std::memcmp(out.get(), out0.get(), 2 * m * sizeof(rt_ray_hit)) != 0;
  }
  // 4) n = 0 and the argument errors
  {
    Scene sc = scene(rng, 3, 0.0f);
    rt_ray r1 = make_ray(0, 0, 0, 0, 0, 0, -1, INFINITY);
    rt_ray_hit h1;
    uint8_t o1;
    bad += rays_host_pass(&sc.c, nullptr, nullptr, 0, nullptr, &why) != RT_OK;
    bad += occluded_host_pass(&sc.c, nullptr, nullptr, 0, nullptr, &why) != RT_OK;
    bad += rays_host_pass(nullptr, &r1, nullptr, 1, &h1, &why) != RT_E_ARG || !why;
    bad += rays_host_pass(&sc.c, nullptr, nullptr, 1, &h1, &why) != RT_E_ARG || !why;
    bad += rays_host_pass(&sc.c, &r1, nullptr, 1, nullptr, &why) != RT_E_ARG || !why;
    bad += occluded_host_pass(nullptr, &r1, nullptr, 1, &o1, &why) != RT_E_ARG || !why;
    bad += occluded_host_pass(&sc.c, nullptr, nullptr, 1, &o1, &why) != RT_E_ARG || !why;
    bad += occluded_host_pass(&sc.c, &r1, nullptr, 1, nullptr, &why) != RT_E_ARG || !why;
    bad += rays_host_pass(&sc.c, &r1, nullptr, static_cast<size_t>(1) << 31, &h1, &why) != RT_E_ARG || !why;
    rt_scene neg{};
    neg.n = -1;
    bad += rays_host_pass(&neg, &r1, nullptr, 1, &h1, &why) != RT_E_ARG || !why;
    calls += 10;
  }
  std::printf("{\"calls\": %ld, \"rays\": %ld, \"hits\": %ld, \"inactive\": %ld, \"guarded\": %ld, \"bad\": %ld}\n", calls,
              rays_all, hits, inactive, guarded, bad);
  return bad ? 1 : 0;
}

// ------------------------------------------------- walk against scan ----
struct HostStack {
  unsigned v[kBvhStack];
  int n = 0;
  bool over = false;
  void push(unsigned node) {
    if (n == kBvhStack) {
      over = true;
      return;
    }
    v[n++] = node;
  }
  bool pop(unsigned& node) {
    if (n == 0) return false;
    node = v[--n];
    return true;
  }
};

// bvh_build's three trees (2, 4 and 8 bodies per leaf) as the walk reads them
struct Trees {
  BvhHost bvh[3];
  std::vector<char> blob[3];
  FhTree tree[3];
  std::vector<float> geo;
};
void build_trees(const std::vector<float>& sph, Trees* T) {
  const int n = static_cast<int>(sph.size() / 4);
  T->geo.resize(4 * static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) fh_geo(&sph[4 * static_cast<size_t>(i)], &T->geo[4 * static_cast<size_t>(i)]);
  for (int k = 0; k < 3; ++k) {
    bvh_build(sph.data(), n, &T->bvh[k], 2 << k, true);
    const BvhHost& b = T->bvh[k];
    const size_t nb = b.nodes.size() * sizeof(BvhNode), pb = b.pairs.size() * sizeof(float),
                 ib = b.pidx.size() * sizeof(int);
    T->blob[k].assign(nb + pb + ib, 0);
    std::memcpy(T->blob[k].data(), b.nodes.data(), nb);
    std::memcpy(T->blob[k].data() + nb, b.pairs.data(), pb);
    std::memcpy(T->blob[k].data() + nb + pb, b.pidx.data(), ib);
    FhTree& t = T->tree[k];
    t.base = T->blob[k].data();
    t.off_pairs = static_cast<int>(nb);
    t.off_pidx = static_cast<int>(nb + pb);
    t.leaf_pairs = 1 << k;
    t.big_pair0 = b.big_pair0;
    t.n_big_leaves = b.n_big_leaves;
    t.ref_mul = static_cast<int>(sizeof(BvhNode));
    for (int j = 0; j < 3; ++j) t.c[j] = b.center[j];
    t.r = b.radius;
    t.c0 = kPadRmax * b.r_max;
  }
}

struct Tally {
  long long rays = 0, active = 0, hits = 0, guarded_hits = 0, finite_tmax = 0, tmin0 = 0;
  long long mis_walk[3] = {0, 0, 0}, mis_any[3] = {0, 0, 0}, stack_over = 0;
  long long cls[4] = {0, 0, 0, 0};
};

void iso(Rng& rng, double* d) {
  double l2;
  do {
    l2 = 0;
    for (int k = 0; k < 3; ++k) d[k] = rng.sym(), l2 += d[k] * d[k];
  } while (l2 > 1.0 || l2 < 1e-6);
  const double il = 1.0 / std::sqrt(l2);
  for (int k = 0; k < 3; ++k) d[k] *= il;
}

// N query rays on one scene: see the head of this file
void walk_scene(const std::vector<float>& sph, long long n_rays, Rng& rng, Tally* tl) {
  const int n = static_cast<int>(sph.size() / 4);
  Trees T;
  build_trees(sph, &T);
  // the bodies a ray can aim at (finite, a radius of its own), and their box
  // without the grounds (r > 50), which would make every origin a far one
  std::vector<int> aim;
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int pass = 0; pass < 2 && aim.empty(); ++pass)
    for (int b = 0; b < n; ++b) {
      const float* q = &sph[4 * static_cast<size_t>(b)];
      if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]) && std::isfinite(q[3]))) continue;
      if (pass == 0 && std::fabs(q[3]) > 50.0f) continue;
      aim.push_back(b);
      for (int k = 0; k < 3; ++k) {
        lo[k] = std::fmin(lo[k], static_cast<double>(q[k]) - std::fabs(q[3]));
        hi[k] = std::fmax(hi[k], static_cast<double>(q[k]) + std::fabs(q[3]));
      }
    }
  if (aim.empty()) {
    aim.push_back(-1);
    for (int k = 0; k < 3; ++k) lo[k] = -1.0, hi[k] = 1.0;
  }
  for (long long i = 0; i < n_rays; ++i) {
    const int cls = static_cast<int>(i & 3);
    const int b = aim[rng.next() % aim.size()];
    const float none4[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    const float* q = b >= 0 ? &sph[4 * static_cast<size_t>(b)] : none4;
    const double rad = std::fabs(static_cast<double>(q[3]));
    double o[3], d[3], aimp[3];
    for (int k = 0; k < 3; ++k) aimp[k] = q[k] + 1.5 * rad * rng.sym();
    int last = -1;
    if (cls == 0 || cls == 1) {
      // 0: in the box grown twofold; 1: far outside, the box grown 60-fold
      const double grow = cls == 0 ? 2.0 : 60.0;
      for (int k = 0; k < 3; ++k) {
        const double c = 0.5 * (lo[k] + hi[k]), h = 0.5 * (hi[k] - lo[k]) * grow;
        o[k] = c + h * rng.sym();
        d[k] = aimp[k] - o[k];
      }
      if (rng.unit() < 0.15) last = static_cast<int>(rng.next() % static_cast<uint64_t>(n + 1));
    } else if (cls == 2) {
      // deep inside a body, any direction
      double v[3];
      iso(rng, v);
      const double f = 0.6 * rng.unit();
      for (int k = 0; k < 3; ++k) o[k] = q[k] + f * rad * v[k];
      iso(rng, d);
      if (rng.unit() < 0.15) last = b;
    } else {
      // on a surface (as fp32 puts it there), any direction, mostly guarded
      double v[3];
      iso(rng, v);
      for (int k = 0; k < 3; ++k) o[k] = q[k] + rad * v[k];
      iso(rng, d);
      if (rng.unit() < 0.8) last = b;
    }
    double len = 0;
    for (int k = 0; k < 3; ++k) len += d[k] * d[k];
    len = std::sqrt(len);
    const double want = std::exp2(12.0 * rng.unit() - 6.0);   // |d| log-uniform in 2^-6 .. 2^6
    rt_ray r;
    for (int k = 0; k < 3; ++k) {
      r.o[k] = static_cast<float>(o[k]);
      r.d[k] = static_cast<float>(d[k] / (len > 0 ? len : 1.0) * want);
    }
    if (i % 16 == 5) r.d[rng.next() % 3] = (i % 32 == 5) ? 0.0f : -0.0f;
    const double u3 = rng.unit();
    r.t_min = u3 < 0.4 ? 0.0f : u3 < 0.7 ? 1e-3f : static_cast<float>(0.1 * rng.unit());
    // the target's parameter in |d| units; half the rays unbounded
    double dist = 0;
    for (int k = 0; k < 3; ++k) dist += (aimp[k] - o[k]) * (aimp[k] - o[k]);
    const double t_aim = (cls <= 1 ? std::sqrt(dist) : rad) / want;
    r.t_max = rng.unit() < 0.5 ? INFINITY : static_cast<float>((0.5 + rng.unit()) * t_aim);
    ++tl->rays;
    ++tl->cls[cls];
    FhRay fr;
    float tbest;
    if (!rq_ray(r.o[0], r.o[1], r.o[2], r.t_min, r.d[0], r.d[1], r.d[2], r.t_max, fr, tbest)) continue;
    ++tl->active;
    last = rq_guard(T.geo.data(), n, last);   // (a body without a disc is no guard: rt.h's step 3)
    tl->finite_tmax += std::isfinite(tbest);
    tl->tmin0 += r.t_min == 0.0f;
    FhBest ref{tbest, -1};
    fh_scan<true>(fr, T.geo.data(), n, ref, last);
    tl->hits += ref.body >= 0;
    tl->guarded_hits += ref.body >= 0 && ref.body == last;
    const bool any_scan = rq_scan_any(fr, T.geo.data(), n, tbest, last);
    if (any_scan != (ref.body >= 0)) ++tl->mis_any[0];
    for (int k = 0; k < 3; ++k) {
      HostStack st;
      FhBest got{tbest, -1};
      fh_walk<true>(fr, T.tree[k], st, got, last);
      if (got.body != ref.body || bits(got.t) != bits(ref.t)) {
        if (tl->mis_walk[k]++ < 3)   // the first few, for whoever reads the failure
          std::fprintf(stderr,
                       "walk != scan, tree %d: o %a %a %a t_min %a d %a %a %a t_max %a last %d class %d: scan %d %a walk %d %a\n",
                       k, r.o[0], r.o[1], r.o[2], r.t_min, r.d[0], r.d[1], r.d[2], r.t_max, last, cls, ref.body, ref.t,
                       got.body, got.t);
      }
      tl->stack_over += st.over;
      HostStack st2;
      const bool any = fh_walk_any<true>(fr, T.tree[k], st2, tbest, last);
      if (any != (ref.body >= 0)) ++tl->mis_any[k];
      tl->stack_over += st2.over;
    }
  }
}

bool read_floats(const char* path, size_t per, std::vector<float>* out) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  bool ok = bytes >= 0 && static_cast<size_t>(bytes) % (per * sizeof(float)) == 0;
  if (ok) {
    out->resize(static_cast<size_t>(bytes) / sizeof(float));
    ok = out->empty() || std::fread(out->data(), sizeof(float), out->size(), f) == out->size();
  }
  std::fclose(f);
  return ok;
}

int walk_run(long long n_rays, uint64_t seed, const char* scene_path) {
  Rng rng{seed};
  std::vector<std::vector<float>> scenes;
  if (scene_path) {
    std::vector<float> sph;
    if (!read_floats(scene_path, 4, &sph) || sph.size() / 4 > RT_MAX_SPHERES) {
      std::fprintf(stderr, "rays_check: cannot read %s (n x 4 floats, n <= %d)\n", scene_path, RT_MAX_SPHERES);
      return 2;
    }
    scenes.push_back(sph);
  } else {
    const int cap = RT_MAX_SPHERES;
    std::vector<float> sph(4 * cap), mat(4 * cap);
    std::vector<int> kind(cap);
    int n = rt_scene_reference(sph.data(), kind.data(), mat.data(), cap);
    scenes.emplace_back(sph.begin(), sph.begin() + 4 * n);
    for (int grid : {11, 16}) {
      n = rt_scene_cover(grid, 42, sph.data(), kind.data(), mat.data(), cap);
      scenes.emplace_back(sph.begin(), sph.begin() + 4 * n);
    }
  }
  Tally tl;
  std::printf("{\"bodies\": [");
  for (size_t s = 0; s < scenes.size(); ++s) {
    walk_scene(scenes[s], n_rays, rng, &tl);
    std::printf("%s%zu", s ? ", " : "", scenes[s].size() / 4);
  }
  std::printf(
      "], \"rays\": %lld, \"active\": %lld, \"hits\": %lld, \"guarded_hits\": %lld, \"finite_tmax\": %lld, \"tmin0\": %lld, "
      "\"classes\": [%lld, %lld, %lld, %lld], \"mismatch_walk\": [%lld, %lld, %lld], \"mismatch_any\": [%lld, %lld, %lld], "
      "\"stack_over\": %lld}\n",
      tl.rays, tl.active, tl.hits, tl.guarded_hits, tl.finite_tmax, tl.tmin0, tl.cls[0], tl.cls[1], tl.cls[2], tl.cls[3],
      tl.mis_walk[0], tl.mis_walk[1], tl.mis_walk[2], tl.mis_any[0], tl.mis_any[1], tl.mis_any[2], tl.stack_over);
  long long bad = tl.stack_over;
  for (int k = 0; k < 3; ++k) bad += tl.mis_walk[k] + tl.mis_any[k];
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "walk")) {
    if (argc < 4) {
      std::fprintf(stderr, "usage: rays_check | rays_check walk N SEED [--scene FILE]\n");
      return 2;
    }
    const char* scene_path = argc >= 6 && !std::strcmp(argv[4], "--scene") ? argv[5] : nullptr;
    return walk_run(std::atoll(argv[2]), std::strtoull(argv[3], nullptr, 10), scene_path);
  }
  return sanitizer_run();
}
