// motion_check — the body-id pass and the motion-aware temporal step
// (csrc/body_ids.h: ids_host_pass and body_motion, the bodies of rt_ids_host
// and rt_body_motion, with the ray and the search ids_kernel runs;
// csrc/temporal.h: tp_host_step_motion, the body of rt_temporal_host_motion,
// with tp_motion and tp_pixel, the text temporal_step_motion_kernel runs) built
// for the host under the sanitizers, over inputs rt.h leaves unspecified: the
// numbers may be anything, the indices may not.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all -static-libasan -static-libubsan tools/motion_check.cpp
//
// Every array is a heap block of exactly its size, so a read outside the
// motion table or a tap outside the image is a report.  Inputs: cameras that
// are ordinary, NaN, infinite and all zero; scenes with NaN, infinite, zero,
// negative and 3e38 centres and radii; ids far out of range, INT32_MIN and
// INT32_MAX among them; NaN, infinite and 2^40 displacements; n_bodies = 0.
// One JSON line; exit status 0 when every call returned what it should, every
// id lies in [-1, n) and every length in [1, max_history].
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../include/rt.h"
#include "../raytracing-clj_amd/csrc/body_ids.h"

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
  float uni() { return static_cast<float>(next() >> 40) * 0x1p-24f; }
};

const float kOdd[] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, -1.0f, -4.0f, 1e-42f, 3e38f, -3e38f, 0x1p40f, -0x1p40f};
const int32_t kOddId[] = {INT32_MIN, INT32_MAX, -1, -2, 1 << 30, -(1 << 30), 65536, 0x7ffffff0};

float draw(Rng& r, float lo, float hi, float p) {
  if (r.uni() < p) return kOdd[r.next() % (sizeof kOdd / sizeof kOdd[0])];
  return lo + (hi - lo) * r.uni();
}

template <class T>
std::unique_ptr<T[]> block(size_t n) {
  return std::unique_ptr<T[]>(new T[n]);
}

rt_camera pinhole(int width, int rows, float cx, float cy, float cz, float pixel, float focus) {
  rt_camera c{};
  c.center[0] = cx;
  c.center[1] = cy;
  c.center[2] = cz;
  c.du[0] = pixel;
  c.dv[1] = -pixel;
  c.p00[0] = cx - 0.5f * static_cast<float>(width) * pixel;
  c.p00[1] = cy + 0.5f * static_cast<float>(rows) * pixel;
  c.p00[2] = cz - focus;
  return c;
}

std::vector<rt_camera> cameras(int width, int rows) {
  std::vector<rt_camera> v;
  const rt_camera cur = pinhole(width, rows, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
  v.push_back(cur);
  v.push_back(pinhole(width, rows, 0.03f, -0.02f, 0.0f, 0.01f, 1.0f));
  v.push_back(pinhole(width, rows, 0x1p40f, 0.0f, 0x1p40f, 0.01f, 1.0f));
  rt_camera odd = cur;
  odd.center[1] = NAN;
  v.push_back(odd);
  odd = cur;
  odd.du[0] = INFINITY;
  v.push_back(odd);
  odd = cur;
  odd.p00[0] = 3e38f;
  odd.dv[1] = 3e38f;
  v.push_back(odd);
  v.push_back(rt_camera{});   // all zero: every direction is the zero vector
  return v;
}

struct Scene {
  int n;
  std::unique_ptr<float[]> sphere, mat;
  std::unique_ptr<int[]> kind;
  rt_scene c;
};
Scene scene(Rng& rng, int n, float p_odd) {
  Scene s{n, block<float>(4 * static_cast<size_t>(n)), block<float>(4 * static_cast<size_t>(n)),
          block<int>(static_cast<size_t>(n)), rt_scene{}};
  for (int b = 0; b < n; ++b) {
    for (int c = 0; c < 2; ++c) s.sphere[4 * b + c] = draw(rng, -1.5f, 1.5f, p_odd);
    s.sphere[4 * b + 2] = draw(rng, -8.0f, -2.0f, p_odd);
    s.sphere[4 * b + 3] = draw(rng, 0.05f, 0.6f, p_odd);
    for (int c = 0; c < 4; ++c) s.mat[4 * b + c] = draw(rng, 0.0f, 1.0f, p_odd);
    s.kind[b] = static_cast<int>(rng.next() % 4);
  }
  s.c.n = n;
  s.c.sphere = n ? s.sphere.get() : nullptr;
  s.c.mat_kind = n ? s.kind.get() : nullptr;
  s.c.mat = n ? s.mat.get() : nullptr;
  return s;
}

}  // namespace

int main() {
  Rng rng{2468};
  const int sizes[][2] = {{1, 1}, {1, 7}, {1, 300}, {300, 1}, {9, 13}, {4, 64}, {5, 65}};   // rows x width
  long id_calls = 0, id_pixels = 0, id_hits = 0, bad_id = 0, bad_status = 0;
  long motion_calls = 0, motion_nan = 0;
  long step_calls = 0, degenerate = 0, step_pixels = 0, bad_len = 0, accepted = 0;
  const char* why = nullptr;

  // ---- the id pass -------------------------------------------------------------
  for (const auto& sz : sizes) {
    const int rows = sz[0], width = sz[1];
    const size_t n_px = static_cast<size_t>(rows) * width;
    for (const int row0 : {0, 5, 0x7fffffff - rows})
      for (const rt_camera& cam : cameras(width, rows))
        for (const int n : {0, 1, 5, 40})
          for (const float p_odd : {0.0f, 0.3f, 1.0f}) {
            const Scene s = scene(rng, n, p_odd);
            auto ids = block<int32_t>(n_px);
            for (size_t i = 0; i < n_px; ++i) ids[i] = 0x7fffffff;
            const int rc = ids_host_pass(&s.c, &cam, width, rows, row0, ids.get(), &why);
            ++id_calls;
            if (rc != RT_OK) ++bad_status;
            for (size_t i = 0; i < n_px; ++i) {
              ++id_pixels;
              if (!(ids[i] >= -1 && ids[i] < n)) ++bad_id;
              if (ids[i] >= 0) ++id_hits;
              // a body that is hit has a finite radius whose square is finite
              if (ids[i] >= 0 && ids[i] < n && !(std::fabs(s.sphere[4 * ids[i] + 3] * s.sphere[4 * ids[i] + 3]) < INFINITY))
                ++bad_id;
            }
          }
  }
  {   // the refusals
    const Scene s = scene(rng, 3, 0.0f);
    const rt_camera cam = pinhole(4, 4, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
    int32_t one[16];
    const rt_scene neg{-1, nullptr, nullptr, nullptr};
    if (ids_host_pass(nullptr, &cam, 4, 4, 0, one, &why) != RT_E_ARG || ids_host_pass(&s.c, nullptr, 4, 4, 0, one, &why) != RT_E_ARG ||
        ids_host_pass(&s.c, &cam, 4, 4, 0, nullptr, &why) != RT_E_ARG || ids_host_pass(&s.c, &cam, 0, 4, 0, one, &why) != RT_E_ARG ||
        ids_host_pass(&s.c, &cam, 4, -1, 0, one, &why) != RT_E_ARG || ids_host_pass(&s.c, &cam, 4, 4, -1, one, &why) != RT_E_ARG ||
        ids_host_pass(&s.c, &cam, 1 << 16, 1 << 16, 0, one, &why) != RT_E_ARG || ids_host_pass(&neg, &cam, 4, 4, 0, one, &why) != RT_E_ARG)
      ++bad_status;
    id_calls += 8;
  }

  // ---- the displacement --------------------------------------------------------
  for (const int n : {0, 1, 5, 40})
    for (const float p_odd : {0.0f, 0.3f, 1.0f}) {
      const Scene a = scene(rng, n, p_odd);
      Scene b = scene(rng, n, p_odd);
      for (int k = 0; k < n; ++k)   // most bodies keep their radius and material
        if (k % 3) {
          b.sphere[4 * k + 3] = a.sphere[4 * k + 3];
          b.kind[k] = a.kind[k];
          for (int c = 0; c < 4; ++c) b.mat[4 * k + c] = a.mat[4 * k + c];
        }
      auto out = block<float>(4 * static_cast<size_t>(n));
      if (body_motion(&a.c, &b.c, out.get(), &why) != RT_OK) ++bad_status;
      ++motion_calls;
      for (int k = 0; k < n; ++k) {
        if (out[4 * k + 3] != 0.0f) ++bad_status;
        if (std::isnan(out[4 * k])) ++motion_nan;
      }
      const Scene other = scene(rng, n + 1, 0.0f);
      if (body_motion(&a.c, &other.c, out.get(), &why) != RT_E_ARG || body_motion(&a.c, nullptr, out.get(), &why) != RT_E_ARG ||
          body_motion(nullptr, &a.c, out.get(), &why) != RT_E_ARG || body_motion(&a.c, &a.c, nullptr, &why) != RT_E_ARG)
        ++bad_status;
      motion_calls += 4;
    }

  // ---- the motion-aware step -----------------------------------------------------
  for (const auto& sz : sizes) {
    const int rows = sz[0], width = sz[1];
    const size_t n = static_cast<size_t>(rows) * width;
    for (const int row0 : {0, 5, 0x7fffffff - rows}) {
      const rt_camera cur = pinhole(width, rows, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
      std::vector<rt_camera> prevs = cameras(width, rows);
      for (int k = 28; k <= 34; k += 3) {   // fx, fy of the order +-2^k pixels, through +-2^31
        prevs.push_back(pinhole(width, rows, 1.0f, 1.0f, 0.0f, std::ldexp(1.0f, -k), 1.0f));
        prevs.push_back(pinhole(width, rows, -1.0f, -1.0f, 0.0f, std::ldexp(1.0f, -k), 1.0f));
      }
      for (const rt_camera& prev : prevs)
        for (const int n_bodies : {0, 1, 7})
          for (const float p_odd : {0.0f, 0.3f, 1.0f}) {
            auto half0 = block<float>(3 * n), half1 = block<float>(3 * n), feat = block<float>(8 * n), a0 = block<float>(3 * n),
                 a1 = block<float>(3 * n), guide = block<float>(4 * n), len = block<float>(n), out0 = block<float>(3 * n),
                 out1 = block<float>(3 * n), out_len = block<float>(n);
            auto ids = block<int32_t>(n);
            auto motion = block<float>(4 * static_cast<size_t>(n_bodies));
            for (size_t i = 0; i < 3 * n; ++i) {
              half0[i] = draw(rng, 0.0f, 2.0f, p_odd);
              half1[i] = draw(rng, 0.0f, 2.0f, p_odd);
              a0[i] = draw(rng, 0.0f, 2.0f, p_odd);
              a1[i] = draw(rng, 0.0f, 2.0f, p_odd);
            }
            for (size_t i = 0; i < n; ++i) {
              for (int c = 0; c < 8; ++c) feat[8 * i + c] = draw(rng, -1.0f, 1.0f, p_odd);
              feat[8 * i + 6] = draw(rng, 0.5f, 30.0f, p_odd > 0.0f ? 0.5f : 0.1f);
              for (int c = 0; c < 3; ++c) guide[4 * i + c] = p_odd > 0.0f ? draw(rng, -1.0f, 1.0f, p_odd) : feat[8 * i + 3 + c];
              guide[4 * i + 3] = draw(rng, 0.5f, 30.0f, p_odd > 0.0f ? 0.5f : 0.1f);
              len[i] = draw(rng, 0.0f, 40.0f, p_odd);
              ids[i] = rng.uni() < 0.3f ? kOddId[rng.next() % (sizeof kOddId / sizeof kOddId[0])]
                                        : static_cast<int32_t>(rng.next() % 12) - 3;
            }
            for (int i = 0; i < 4 * n_bodies; ++i) motion[i] = draw(rng, -0.02f, 0.02f, p_odd > 0.0f ? 0.4f : 0.1f);
            rt_temporal_opts o = tp_default_opts();
            o.sigma_z = p_odd > 0.0f ? 3e38f : 0.1f;
            o.normal_min = p_odd > 0.0f ? -1.0f : 0.9f;
            const int rc = tp_host_step_motion(&o, &cur, &prev, width, rows, row0, half0.get(), half1.get(), feat.get(),
                                               a0.get(), a1.get(), guide.get(), len.get(), ids.get(),
                                               n_bodies ? motion.get() : nullptr, n_bodies, out0.get(), out1.get(),
                                               out_len.get(), &why);
            ++step_calls;
            float R[9], dc[3];
            const bool degen = !tp_setup(cur, prev, R, dc);
            degenerate += degen;
            if (rc != (degen ? RT_E_ARG : RT_OK)) ++bad_status;
            if (rc != RT_OK) continue;
            for (size_t i = 0; i < n; ++i) {
              ++step_pixels;
              if (!(out_len[i] >= 1.0f && out_len[i] <= static_cast<float>(o.max_history))) ++bad_len;
              if (out_len[i] > 1.0f) ++accepted;
            }
          }
    }
  }
  {   // the refusals of the new arguments
    float h[3] = {0, 0, 0}, f[8] = {0, 0, 0, 0, 0, 1, 5, 1}, o0[3], o1[3], ol[1], m[4] = {0, 0, 0, 0};
    int32_t id[1] = {0};
    const rt_camera cur = pinhole(1, 1, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
    auto call = [&](const int32_t* ids, const float* motion, int nb) {
      ++step_calls;
      return tp_host_step_motion(nullptr, &cur, nullptr, 1, 1, 0, h, h, f, nullptr, nullptr, nullptr, nullptr, ids, motion, nb,
                                 o0, o1, ol, &why);
    };
    if (call(id, m, 1) != RT_OK || call(id, nullptr, 0) != RT_OK || call(nullptr, m, 1) != RT_E_ARG ||
        call(id, m, -1) != RT_E_ARG || call(id, nullptr, 1) != RT_E_ARG)
      ++bad_status;
  }
  std::printf("{\"id_calls\": %ld, \"id_pixels\": %ld, \"id_hits\": %ld, \"bad_id\": %ld, \"motion_calls\": %ld, "
              "\"motion_nan\": %ld, \"step_calls\": %ld, \"degenerate\": %ld, \"step_pixels\": %ld, \"bad_len\": %ld, "
              "\"accepted\": %ld, \"bad_status\": %ld}\n",
              id_calls, id_pixels, id_hits, bad_id, motion_calls, motion_nan, step_calls, degenerate, step_pixels, bad_len,
              accepted, bad_status);
  return bad_status == 0 && bad_id == 0 && bad_len == 0 && id_hits > 0 && accepted > 0 && degenerate > 0 && motion_nan > 0 ? 0 : 1;
}
