// temporal_check — temporal accumulation's step (csrc/temporal.h: tp_host_step,
// the body of rt_temporal_host, and tp_pixel, the text temporal_step_kernel
// runs) built for the host under the sanitizers, over inputs rt.h leaves
// unspecified: the numbers may be anything, the indices may not.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all -static-libasan -static-libubsan tools/temporal_check.cpp
//
// Every array is a heap block of exactly its size, so a tap outside the image
// is a report.  Inputs: colours, guides, depths and history lengths drawn from
// ordinary values mixed with NaN, +-inf, 0, negatives, denormals and 3e38;
// images of 1 x 1, 1 x N, N x 1 and a few more, row0 of 0, 5 and the largest
// legal one; camera pairs that are still, shifted, 2^40 apart, scaled so that
// fx and fy sweep through +-2^31, looking backwards, NaN, and degenerate
// (det = 0: RT_E_ARG expected).  One JSON line; exit status 0 when every call
// returned what it should and every length lies in [1, max_history].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
  Rng rng{12345};
  const int sizes[][2] = {{1, 1}, {1, 7}, {1, 300}, {300, 1}, {5, 1}, {9, 13}, {4, 64}, {5, 65}};   // rows x width
  long calls = 0, degenerate = 0, bad_status = 0, bad_len = 0, accepted = 0, pixels = 0;
  for (const auto& sz : sizes) {
    const int rows = sz[0], width = sz[1];
    const size_t n = static_cast<size_t>(rows) * width;
    for (const int row0 : {0, 5, 0x7fffffff - rows}) {
      const rt_camera cur = pinhole(width, rows, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
      std::vector<rt_camera> prevs;
      prevs.push_back(cur);                                                    // still
      prevs.push_back(pinhole(width, rows, 0.03f, -0.02f, 0.0f, 0.01f, 1.0f));   // a few pixels
      prevs.push_back(pinhole(width, rows, 0x1p40f, 0.0f, 0x1p40f, 0.01f, 1.0f));   // 2^40 apart
      prevs.push_back(pinhole(width, rows, 0.0f, 0.0f, -50.0f, 0.01f, 1.0f));   // behind the old image plane
      for (int k = 20; k <= 34; ++k) {   // fx, fy of the order +-2^k pixels, through +-2^31
        prevs.push_back(pinhole(width, rows, 1.0f, 1.0f, 0.0f, std::ldexp(1.0f, -k), 1.0f));
        prevs.push_back(pinhole(width, rows, -1.0f, -1.0f, 0.0f, std::ldexp(1.0f, -k), 1.0f));
      }
      rt_camera odd = cur;
      odd.center[1] = NAN;
      prevs.push_back(odd);
      odd = cur;
      odd.du[0] = INFINITY;
      prevs.push_back(odd);
      odd = cur;
      odd.du[0] = 0.0f;   // det = 0
      prevs.push_back(odd);
      odd = cur;
      odd.p00[0] = 3e38f;
      odd.dv[1] = 3e38f;
      prevs.push_back(odd);
      for (const rt_camera& prev : prevs)
        for (const float p_odd : {0.0f, 0.3f, 1.0f}) {
          auto half0 = block(3 * n), half1 = block(3 * n), feat = block(8 * n), a0 = block(3 * n), a1 = block(3 * n),
               guide = block(4 * n), len = block(n), out0 = block(3 * n), out1 = block(3 * n), out_len = block(n);
          for (size_t i = 0; i < 3 * n; ++i) {
            half0[i] = draw(rng, 0.0f, 2.0f, p_odd);
            half1[i] = draw(rng, 0.0f, 2.0f, p_odd);
            a0[i] = draw(rng, 0.0f, 2.0f, p_odd);
            a1[i] = draw(rng, 0.0f, 2.0f, p_odd);
          }
          for (size_t i = 0; i < n; ++i) {
            for (int c = 0; c < 8; ++c) feat[8 * i + c] = draw(rng, -1.0f, 1.0f, p_odd);
            feat[8 * i + 6] = draw(rng, 0.5f, 30.0f, p_odd > 0.0f ? 0.5f : 0.1f);   // depths: NaN, <= 0, +-inf among them
            for (int c = 0; c < 3; ++c) guide[4 * i + c] = p_odd > 0.0f ? draw(rng, -1.0f, 1.0f, p_odd) : feat[8 * i + 3 + c];
            guide[4 * i + 3] = draw(rng, 0.5f, 30.0f, p_odd > 0.0f ? 0.5f : 0.1f);
            len[i] = draw(rng, 0.0f, 40.0f, p_odd);
          }
          rt_temporal_opts o = tp_default_opts();
          o.sigma_z = p_odd > 0.0f ? 3e38f : 0.1f;   // (3e38 * zexp overflows: every finite depth passes)
          o.normal_min = p_odd > 0.0f ? -1.0f : 0.9f;
          const char* why = nullptr;
          const int rc = tp_host_step(&o, &cur, &prev, width, rows, row0, half0.get(), half1.get(), feat.get(), a0.get(),
                                      a1.get(), guide.get(), len.get(), out0.get(), out1.get(), out_len.get(), &why);
          ++calls;
          float R[9], dc[3];
          const bool degen = !tp_setup(cur, prev, R, dc);
          degenerate += degen;
          if (rc != (degen ? RT_E_ARG : RT_OK)) ++bad_status;
          if (rc != RT_OK) continue;
          for (size_t i = 0; i < n; ++i) {
            ++pixels;
            if (!(out_len[i] >= 1.0f && out_len[i] <= static_cast<float>(o.max_history))) ++bad_len;
            if (out_len[i] > 1.0f) ++accepted;
          }
        }
    }
  }
  // no previous camera: the history arrays are not read
  {
    auto half0 = block(3), half1 = block(3), feat = block(8), out0 = block(3), out1 = block(3), out_len = block(1);
    for (int c = 0; c < 3; ++c) half0[c] = half1[c] = NAN;
    for (int c = 0; c < 8; ++c) feat[c] = NAN;
    const rt_camera cur = pinhole(1, 1, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
    const char* why = nullptr;
    const int rc = tp_host_step(nullptr, &cur, nullptr, 1, 1, 0, half0.get(), half1.get(), feat.get(), nullptr, nullptr,
                                nullptr, nullptr, out0.get(), out1.get(), out_len.get(), &why);
    ++calls;
    if (rc != RT_OK || out_len[0] != 1.0f) ++bad_status;
  }
  std::printf("{\"calls\": %ld, \"degenerate\": %ld, \"bad_status\": %ld, \"pixels\": %ld, \"bad_len\": %ld, "
              "\"accepted\": %ld}\n",
              calls, degenerate, bad_status, pixels, bad_len, accepted);
  return bad_status == 0 && bad_len == 0 && accepted > 0 && degenerate > 0 ? 0 : 1;
}
