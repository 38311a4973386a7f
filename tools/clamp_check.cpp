// clamp_check — the colour clamp of temporal accumulation (csrc/temporal.h:
// tp_host_step_clamp, the body of rt_temporal_host_clamp, with tp_clamp_box,
// the text temporal_box_kernel runs, and tp_pixel<MOTION, CLAMP>) built for the
// host under the sanitizers, over inputs rt.h leaves unspecified: the numbers
// may be anything, the indices may not.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all -static-libasan -static-libubsan tools/clamp_check.cpp
//
// Every array is a heap block of exactly its size, so a tap outside the band
// is a report.  Inputs: colours, guides, depths and history lengths drawn from
// ordinary values mixed with NaN, +-inf, 0, negatives, denormals and 3e38 (NaN
// and infinite colours; NaN, zero and negative depths); radius 1..3 on images
// of 1 x 1, 1 x 7, 7 x 1 and a few more, row0 of 0, 5 and the largest legal
// one; gamma ordinary, +inf and denormal; with and without ids; radii and
// gammas outside the ranges (RT_E_ARG expected, nothing written).  With
// gamma = +inf the outputs' bits must be the unclamped step's on every input.
// One JSON line; exit status 0 when every call returned what it should, every
// length lies in [1, max_history] and the identity held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../include/rt.h"
#include "../raytracing-clj_amd/csrc/temporal.h"

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

const float kOdd[] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, -1.0f, -4.0f, 1e-42f, 3e38f, -3e38f, 0x1p31f, -0x1p31f};

// an ordinary value in [lo, hi), or with probability p one of kOdd
float draw(Rng& r, float lo, float hi, float p) {
  if (r.uni() < p) return kOdd[r.next() % (sizeof kOdd / sizeof kOdd[0])];
  return lo + (hi - lo) * r.uni();
}

// exactly n floats on the heap (no slack behind them)
std::unique_ptr<float[]> block(size_t n) { return std::unique_ptr<float[]>(new float[n]); }

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

}  // namespace

int main() {
  Rng rng{2468};
  const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {1, 300}, {9, 13}, {4, 64}, {5, 65}};   // rows x width
  const float gammas[] = {1.0f, 0.25f, INFINITY, 1e-42f, 3e38f};
  constexpr int kBodies = 5;
  long calls = 0, refused = 0, bad_status = 0, bad_len = 0, accepted = 0, pixels = 0, identity_calls = 0,
       bad_identity = 0;
  for (const auto& sz : sizes) {
    const int rows = sz[0], width = sz[1];
    const size_t n = static_cast<size_t>(rows) * width;
    for (const int row0 : {0, 5, 0x7fffffff - rows}) {
      const rt_camera cur = pinhole(width, rows, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
      const rt_camera prevs[] = {cur, pinhole(width, rows, 0.03f, -0.02f, 0.0f, 0.01f, 1.0f),
                                 pinhole(width, rows, 1.0f, 1.0f, 0.0f, 0x1p-31f, 1.0f)};
      for (const rt_camera& prev : prevs)
        for (const float p_odd : {0.0f, 0.3f, 1.0f})
          for (int radius = 0; radius <= 4; ++radius)
            for (const float gamma : gammas)
              for (const bool with_ids : {false, true}) {
                auto half0 = block(3 * n), half1 = block(3 * n), feat = block(8 * n), a0 = block(3 * n),
                     a1 = block(3 * n), guide = block(4 * n), len = block(n), out0 = block(3 * n), out1 = block(3 * n),
                     out_len = block(n), motion = block(4 * kBodies);
                std::unique_ptr<int32_t[]> ids(new int32_t[n]);
                for (size_t i = 0; i < 3 * n; ++i) {
                  half0[i] = draw(rng, 0.0f, 2.0f, p_odd);
                  half1[i] = draw(rng, 0.0f, 2.0f, p_odd);
                  a0[i] = draw(rng, 0.0f, 2.0f, p_odd);
                  a1[i] = draw(rng, 0.0f, 2.0f, p_odd);
                  out0[i] = out1[i] = 7.0f;
                }
                for (size_t i = 0; i < n; ++i) {
                  for (int c = 0; c < 8; ++c) feat[8 * i + c] = draw(rng, -1.0f, 1.0f, p_odd);
                  if (p_odd == 0.0f) {   // one surface: the windows fill up
                    feat[8 * i + 3] = 0.0f, feat[8 * i + 4] = 0.6f, feat[8 * i + 5] = 0.8f;
                  }
                  // depths: NaN, <= 0, +-inf among them
                  feat[8 * i + 6] = p_odd == 0.0f ? 9.0f + 0.01f * rng.uni() : draw(rng, 0.5f, 30.0f, 0.5f);
                  for (int c = 0; c < 4; ++c) guide[4 * i + c] = p_odd > 0.0f ? draw(rng, 0.5f, 30.0f, p_odd) : feat[8 * i + 3 + c];
                  len[i] = draw(rng, 0.0f, 40.0f, p_odd);
                  ids[i] = static_cast<int32_t>(rng.next() % (kBodies + 6)) - 3;
                  out_len[i] = 7.0f;
                }
                for (int i = 0; i < 4 * kBodies; ++i) motion[i] = draw(rng, -0.05f, 0.05f, p_odd * 0.3f);
                rt_temporal_opts o = tp_default_opts();
                o.sigma_z = p_odd > 0.0f ? 3e38f : 0.1f;
                o.normal_min = p_odd > 0.0f ? -1.0f : 0.9f;
                const rt_temporal_clamp_opts k{radius, gamma};
                const char* why = nullptr;
                const int rc = tp_host_step_clamp(&o, &k, &cur, &prev, width, rows, row0, half0.get(), half1.get(),
                                                  feat.get(), a0.get(), a1.get(), guide.get(), len.get(),
                                                  with_ids ? ids.get() : nullptr, motion.get(), kBodies, out0.get(),
                                                  out1.get(), out_len.get(), &why);
                ++calls;
                const bool bad_opts = radius < 1 || radius > 3;
                if (rc != (bad_opts ? RT_E_ARG : RT_OK)) ++bad_status;
                if (rc != RT_OK) {
                  ++refused;
                  for (size_t i = 0; i < n; ++i)
                    if (out0[3 * i] != 7.0f || out1[3 * i] != 7.0f || out_len[i] != 7.0f) ++bad_status;   // written
                  continue;
                }
                for (size_t i = 0; i < n; ++i) {
                  ++pixels;
                  if (!(out_len[i] >= 1.0f && out_len[i] <= static_cast<float>(o.max_history))) ++bad_len;
                  if (out_len[i] > 1.0f) ++accepted;
                }
                if (gamma == INFINITY) {   // the unclamped step's bits, whatever the inputs
                  auto w0 = block(3 * n), w1 = block(3 * n), wl = block(n);
                  const int rc2 =
                      with_ids ? tp_host_step_motion(&o, &cur, &prev, width, rows, row0, half0.get(), half1.get(),
                                                     feat.get(), a0.get(), a1.get(), guide.get(), len.get(), ids.get(),
                                                     motion.get(), kBodies, w0.get(), w1.get(), wl.get(), &why)
                               : tp_host_step(&o, &cur, &prev, width, rows, row0, half0.get(), half1.get(), feat.get(),
                                              a0.get(), a1.get(), guide.get(), len.get(), w0.get(), w1.get(), wl.get(),
                                              &why);
                  ++identity_calls;
                  if (rc2 != RT_OK || std::memcmp(w0.get(), out0.get(), 3 * n * sizeof(float)) != 0 ||
                      std::memcmp(w1.get(), out1.get(), 3 * n * sizeof(float)) != 0 ||
                      std::memcmp(wl.get(), out_len.get(), n * sizeof(float)) != 0)
                    ++bad_identity;
                }
              }
    }
  }
  // gammas outside the range, NULL options (the defaults), no previous camera
  {
    auto half0 = block(3), half1 = block(3), feat = block(8), out0 = block(3), out1 = block(3), out_len = block(1);
    for (int c = 0; c < 3; ++c) half0[c] = half1[c] = NAN;
    for (int c = 0; c < 8; ++c) feat[c] = NAN;
    const rt_camera cur = pinhole(1, 1, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
    const char* why = nullptr;
    for (const float gamma : {0.0f, -0.0f, -1.0f, NAN, -INFINITY}) {
      const rt_temporal_clamp_opts k{2, gamma};
      out_len[0] = 7.0f;
      const int rc = tp_host_step_clamp(nullptr, &k, &cur, nullptr, 1, 1, 0, half0.get(), half1.get(), feat.get(), nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr, 0, out0.get(), out1.get(),
                                        out_len.get(), &why);
      ++calls;
      ++refused;
      if (rc != RT_E_ARG || out_len[0] != 7.0f) ++bad_status;
    }
    const int rc = tp_host_step_clamp(nullptr, nullptr, &cur, nullptr, 1, 1, 0, half0.get(), half1.get(), feat.get(),
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, out0.get(), out1.get(),
                                      out_len.get(), &why);
    ++calls;
    if (rc != RT_OK || out_len[0] != 1.0f) ++bad_status;
  }
  std::printf("{\"calls\": %ld, \"refused\": %ld, \"bad_status\": %ld, \"pixels\": %ld, \"bad_len\": %ld, "
              "\"accepted\": %ld, \"identity_calls\": %ld, \"bad_identity\": %ld}\n",
              calls, refused, bad_status, pixels, bad_len, accepted, identity_calls, bad_identity);
  return bad_status == 0 && bad_len == 0 && bad_identity == 0 && accepted > 0 && refused > 0 ? 0 : 1;
}
