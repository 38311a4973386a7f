// first_hit_check — the feature pass's hit search (csrc/first_hit.h, the text
// feat_kernel runs) built for the host: for every ray the stack walk over
// each of bvh_build's three trees must return the linear scan's (body, t
// bits).  tests/test_first_hit_walk.py runs it and reads the one JSON line.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -mfma -Icsrc tools/first_hit_check.cpp csrc/bvh.cpp csrc/scenes.cpp
//
// Scenes: rt_scene_cover(11, seed), the reference's five bodies, and 64 bodies
// in which every body appears twice (index i and i + 32: every hit is a tie
// the lower index must win).  Rays per scene: camera rays of the cover camera
// and of the reference camera (jittered pixels, defocus disk), and as many
// rays with origins inside the tree's bounding sphere and isotropic
// directions, every fourth with one or two components exactly zero.
//
//   first_hit_check --scene FILE --rays FILE
// The same checks -- walk equals scan over the three trees, the stack within
// depth - 1, and that it ends -- for a caller's inputs, raw little-endian
// float32: bodies as n x (cx, cy, cz, r), rays as m x (o, d).  Non-finite
// bodies and rays are inputs like any other (tests/test_first_hit_walk.py
// feeds the edge scenes' bodies and the oracle's camera rays).  Another JSON
// line; exit status 1 on a mismatch, 2 on unreadable input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/rt.h"
#include "../raytracing-clj_amd/csrc/bvh.h"
#include "../raytracing-clj_amd/csrc/first_hit.h"

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
};

struct Ray {
  float o[3], d[3];
};

struct Cam {
  double from[3], at[3], vfov, defocus, focus;
};
const Cam kCoverCam = {{13, 2, 3}, {0, 0, 0}, 20.0, 0.6, 10.0};
const Cam kRefCam = {{-2, 2, 1}, {0, 0, -1}, 20.0, 10.0, 3.4};

// compute-pixel's ray (raytracing.clj:117-151) in double, rounded to float
void camera_rays(const Cam& c, int w, int h, int spp, Rng& rng, std::vector<Ray>* out) {
  const double pi = 3.141592653589793;
  auto sub = [](const double* a, const double* b, double* r) { for (int k = 0; k < 3; ++k) r[k] = a[k] - b[k]; };
  auto cross = [](const double* a, const double* b, double* r) {
    r[0] = a[1] * b[2] - a[2] * b[1], r[1] = a[2] * b[0] - a[0] * b[2], r[2] = a[0] * b[1] - a[1] * b[0];
  };
  auto unit = [](double* a) {
    const double l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int k = 0; k < 3; ++k) a[k] /= l;
  };
  const double up[3] = {0, 1, 0};
  double wv[3], u[3], v[3];
  sub(c.from, c.at, wv);
  unit(wv);
  cross(up, wv, u);
  unit(u);
  cross(wv, u, v);
  const double vh = 2.0 * std::tan(c.vfov * pi / 360.0) * c.focus, vw = vh * w / h;
  const double rad = c.focus * std::tan(c.defocus * pi / 360.0);
  for (int j = 0; j < h; ++j)
    for (int i = 0; i < w; ++i)
      for (int s = 0; s < spp; ++s) {
        const double fx = (i + rng.unit()) / w - 0.5, fy = (j + rng.unit()) / h - 0.5;
        double qx, qy;
        do {
          qx = rng.sym(), qy = rng.sym();
        } while (qx * qx + qy * qy >= 1.0);
        Ray r;
        for (int k = 0; k < 3; ++k) {
          const double o = c.from[k] + rad * (qx * u[k] + qy * v[k]);
          const double p = c.from[k] - c.focus * wv[k] + fx * vw * u[k] - fy * vh * v[k];
          r.o[k] = static_cast<float>(o);
          r.d[k] = static_cast<float>(p) - r.o[k];
        }
        out->push_back(r);
      }
}

// origins inside the sphere (c, rad), isotropic directions of length 0.5 .. 2;
// every fourth ray with one or two components exactly zero
void iso_rays(const float* c, float rad, size_t n, Rng& rng, std::vector<Ray>* out) {
  for (size_t i = 0; i < n; ++i) {
    double p[3], d[3], l2;
    do {
      l2 = 0;
      for (int k = 0; k < 3; ++k) p[k] = rng.sym(), l2 += p[k] * p[k];
    } while (l2 > 1.0);
    do {
      l2 = 0;
      for (int k = 0; k < 3; ++k) d[k] = rng.sym(), l2 += d[k] * d[k];
    } while (l2 > 1.0 || l2 < 1e-6);
    const double len = (0.5 + 1.5 * rng.unit()) / std::sqrt(l2);
    Ray r;
    for (int k = 0; k < 3; ++k) {
      r.o[k] = static_cast<float>(c[k] + rad * p[k]);
      r.d[k] = static_cast<float>(d[k] * len);
    }
    if (i % 4 == 0) {
      const int z = static_cast<int>(rng.next() % 3);
      r.d[z] = (i % 8 == 0) ? 0.0f : -0.0f;
      if (i % 16 == 0) r.d[(z + 1) % 3] = 0.0f;
    }
    out->push_back(r);
  }
}

struct HostStack {
  unsigned v[kBvhStack];
  int n = 0, peak = 0;
  bool over = false;
  void push(unsigned node) {
    if (n == kBvhStack) {
      over = true;
      return;
    }
    v[n++] = node;
    peak = n > peak ? n : peak;
  }
  bool pop(unsigned& node) {
    if (n == 0) return false;
    node = v[--n];
    return true;
  }
};

struct Scene {
  const char* name;
  std::vector<float> sph;   // n x 4
  int n() const { return static_cast<int>(sph.size() / 4); }
};

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// bvh_build's three trees (2, 4 and 8 bodies per leaf) as the walk reads them
struct Trees {
  BvhHost bvh[3];
  std::vector<char> blob[3];
  FhTree tree[3];
  std::vector<float> geo;   // n x (cx, cy, cz, -r^2): the scan's
  int max_depth = 0;
};

void build_trees(const std::vector<float>& sph, Trees* T) {
  const int n = static_cast<int>(sph.size() / 4);
  T->geo.resize(4 * static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) T->geo[4 * i + k] = sph[4 * i + k];
    T->geo[4 * i + 3] = -(sph[4 * i + 3] * sph[4 * i + 3]);
  }
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
    T->max_depth = b.depth > T->max_depth ? b.depth : T->max_depth;
  }
}

struct Tally {
  long long mismatches[3] = {0, 0, 0};
  long long stack_over = 0;
  int peak = 0;
};

// one ray: the scan's answer, and every tree's walk held to it
FhBest check_ray(const Trees& T, const FhRay& r, Tally* tl) {
  FhBest ref = fh_none();
  fh_scan(r, T.geo.data(), static_cast<int>(T.geo.size() / 4), ref);
  for (int k = 0; k < 3; ++k) {
    HostStack st;
    FhBest got = fh_none();
    fh_walk(r, T.tree[k], st, got);
    if (got.body != ref.body || bits(got.t) != bits(ref.t) || st.over) ++tl->mismatches[k];
    // the device's stack holds depth + 1 rows: depth - 1 suffice
    if (st.peak > T.bvh[k].depth - 1 && st.peak > 0) ++tl->stack_over;
    tl->peak = st.peak > tl->peak ? st.peak : tl->peak;
  }
  return ref;
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

// --scene FILE --rays FILE: the same checks for a caller's bodies (n x (cx, cy,
// cz, r)) and rays (m x (o, d)), raw little-endian float32
int check_files(const char* scene_path, const char* rays_path) {
  std::vector<float> sph, rays;
  if (!read_floats(scene_path, 4, &sph) || !read_floats(rays_path, 6, &rays) || sph.size() / 4 > RT_MAX_SPHERES) {
    std::fprintf(stderr, "first_hit_check: cannot read %s (n x 4 floats, n <= %d) or %s (m x 6 floats)\n", scene_path,
                 RT_MAX_SPHERES, rays_path);
    return 2;
  }
  Trees T;
  build_trees(sph, &T);
  Tally tl;
  long long hits = 0, odd_rays = 0;
  const size_t m = rays.size() / 6;
  for (size_t i = 0; i < m; ++i) {
    const float* q = &rays[6 * i];
    const FhRay r = fh_ray(q[0], q[1], q[2], q[3], q[4], q[5]);
    // |d| zero, infinite or NaN: a unit direction that is not one
    odd_rays += !(std::isfinite(r.len) && r.len > 0.0f && std::isfinite(r.ux) && std::isfinite(r.uy) &&
                  std::isfinite(r.uz));
    hits += check_ray(T, r, &tl).body >= 0;
  }
  std::printf(
      "{\"bodies\": %d, \"rays\": %zu, \"hits\": %lld, \"misses\": %lld, \"odd_rays\": %lld, \"big_bodies\": %d, "
      "\"tree_nodes\": {\"2\": %zu, \"4\": %zu, \"8\": %zu}, \"mismatches\": {\"2\": %lld, \"4\": %lld, \"8\": %lld}, "
      "\"stack_peak\": %d, \"stack_over_depth\": %lld, \"max_depth\": %d}\n",
      static_cast<int>(sph.size() / 4), m, hits, static_cast<long long>(m) - hits, odd_rays,
      static_cast<int>(T.bvh[1].big.size()), T.bvh[0].nodes.size(), T.bvh[1].nodes.size(), T.bvh[2].nodes.size(),
      tl.mismatches[0], tl.mismatches[1], tl.mismatches[2], tl.peak, tl.stack_over, T.max_depth);
  return (tl.mismatches[0] | tl.mismatches[1] | tl.mismatches[2] | tl.stack_over) ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char *scene_path = nullptr, *rays_path = nullptr;
  for (int i = 1; i + 1 < argc; ++i) {
    if (!std::strcmp(argv[i], "--scene")) scene_path = argv[i + 1];
    if (!std::strcmp(argv[i], "--rays")) rays_path = argv[i + 1];
  }
  if (scene_path || rays_path) {
    if (!scene_path || !rays_path) {
      std::fprintf(stderr, "usage: first_hit_check [seed] | --scene FILE --rays FILE\n");
      return 2;
    }
    return check_files(scene_path, rays_path);
  }
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 42;
  Rng rng{seed};
  std::vector<Scene> scenes(3);
  {
    const int cap = RT_MAX_SPHERES;
    std::vector<float> sph(4 * cap), mat(4 * cap);
    std::vector<int> kind(cap);
    int n = rt_scene_cover(11, seed, sph.data(), kind.data(), mat.data(), cap);
    scenes[0] = {"cover", std::vector<float>(sph.begin(), sph.begin() + 4 * n)};
    n = rt_scene_reference(sph.data(), kind.data(), mat.data(), cap);
    scenes[1] = {"reference", std::vector<float>(sph.begin(), sph.begin() + 4 * n)};
    // 32 bodies around both cameras' targets, each twice
    std::vector<float> dup(4 * 64);
    for (int i = 0; i < 32; ++i) {
      const float b[4] = {static_cast<float>(3.0 * rng.sym()), static_cast<float>(0.2 + 1.5 * rng.unit()),
                          static_cast<float>(3.0 * rng.sym() - 0.5), static_cast<float>(0.15 + 0.6 * rng.unit())};
      for (int k = 0; k < 4; ++k) dup[4 * i + k] = dup[4 * (i + 32) + k] = b[k];
    }
    scenes[2] = {"duplicated", dup};
  }
  long long rays_all = 0, cam_rays = 0, cam_hits = 0, tie_rays = 0, big_hits = 0;
  Tally tl;
  int cover_big = 0, max_depth = 0;
  for (size_t si = 0; si < scenes.size(); ++si) {
    const Scene& sc = scenes[si];
    const int n = sc.n();
    Trees T;
    build_trees(sc.sph, &T);
    const BvhHost* bvh = T.bvh;
    const std::vector<float>& geo = T.geo;
    max_depth = T.max_depth > max_depth ? T.max_depth : max_depth;
    if (si == 0) cover_big = static_cast<int>(bvh[1].big.size());
    std::vector<char> is_big(n, 0);
    for (int i : bvh[1].big) is_big[i] = 1;
    std::vector<Ray> rays;
    camera_rays(kCoverCam, 100, 50, 4, rng, &rays);
    camera_rays(kRefCam, 100, 50, 4, rng, &rays);
    const size_t n_cam = rays.size();
    iso_rays(bvh[0].center, bvh[0].radius, n_cam, rng, &rays);
    for (size_t ri = 0; ri < rays.size(); ++ri) {
      const Ray& q = rays[ri];
      const FhRay r = fh_ray(q.o[0], q.o[1], q.o[2], q.d[0], q.d[1], q.d[2]);
      const FhBest ref = check_ray(T, r, &tl);
      ++rays_all;
      if (ri < n_cam) {
        ++cam_rays;
        cam_hits += ref.body >= 0;
      }
      if (si == 0 && ref.body >= 0 && is_big[ref.body]) ++big_hits;
      if (si == 2 && ref.body >= 0 && ref.body < 32) {
        // the twin alone gives the same t: the lower index decided
        FhBest twin = fh_none();
        fh_test(r, geo[4 * (ref.body + 32)], geo[4 * (ref.body + 32) + 1], geo[4 * (ref.body + 32) + 2],
                geo[4 * (ref.body + 32) + 3], ref.body + 32, twin);
        tie_rays += twin.body >= 0 && bits(twin.t) == bits(ref.t);
      }
    }
  }
  const long long* mismatches = tl.mismatches;
  const long long stack_over = tl.stack_over;
  const int peak = tl.peak;
  std::printf(
      "{\"rays\": %lld, \"camera_rays\": %lld, \"camera_hits\": %lld, \"camera_misses\": %lld, \"tie_rays\": %lld, "
      "\"cover_big_bodies\": %d, \"big_hits\": %lld, \"mismatches\": {\"2\": %lld, \"4\": %lld, \"8\": %lld}, "
      "\"stack_peak\": %d, \"stack_over_depth\": %lld, \"max_depth\": %d}\n",
      rays_all, cam_rays, cam_hits, cam_rays - cam_hits, tie_rays, cover_big, big_hits, mismatches[0], mismatches[1],
      mismatches[2], peak, stack_over, max_depth);
  return (mismatches[0] | mismatches[1] | mismatches[2] | stack_over) ? 1 : 0;
}
