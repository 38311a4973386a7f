// budget_check — the sample budget's host side (csrc/budget.h: bd_host_plan,
// the body of rt_budget_plan_host, with bd_tile_mult, the text
// budget_plan_kernel runs; csrc/temporal.h: tp_host_probe and
// tp_host_step_budget, the bodies of rt_temporal_host_probe and
// rt_temporal_host_budget, with tp_pixel<.., WEIGHT, PROBE>) built for the host
// under the sanitizers, over small constructed inputs and inputs rt.h leaves
// unspecified: the numbers may be anything, the indices may not.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all -static-libasan -static-libubsan tools/budget_check.cpp
//
// Every array is a heap block of exactly its size, so a tap or a tile outside
// the band is a report.  Checked besides: the probe followed by the weighted
// step gives out_len == min(len + wt, max_history) bit for bit; multipliers of
// one give rt_temporal_host_clamp's bits; multipliers outside 1..16 behave as
// their clamped values; the plan lies in 1..max_mult and obeys its constructed
// cases; bad options are refused with nothing written.  One JSON line; exit
// status 0 when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../include/rt.h"
#include "../raytracing-clj_amd/csrc/budget.h"
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

// exactly n items on the heap (no slack behind them)
std::unique_ptr<float[]> block(size_t n) { return std::unique_ptr<float[]>(new float[n]); }
std::unique_ptr<uint32_t[]> ublock(size_t n) { return std::unique_ptr<uint32_t[]>(new uint32_t[n]); }

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

// the same floats bit for bit, a NaN standing for any NaN (which operand's
// payload a NaN result carries is the compiler's choice of operand order, and
// rt.h leaves the numbers of such inputs unspecified)
bool same(const float* a, const float* b, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (std::memcmp(a + i, b + i, sizeof(float)) != 0 && !(a[i] != a[i] && b[i] != b[i])) return false;
  return true;
}

long g_bad = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    ++g_bad;
    std::fprintf(stderr, "budget_check: %s\n", what);
  }
}

// ---- the plan ----
void plan_cases(Rng& rng, long* calls) {
  const char* why = nullptr;
  // constructed: one 8 x 8 tile
  {
    auto len = block(64);
    auto mult = ublock(1);
    rt_budget_opts o{1, 8, 8, 16};
    for (int i = 0; i < 64; ++i) len[i] = 32.0f;
    expect(bd_host_plan(&o, len.get(), 8, 8, mult.get(), &why) == RT_OK && mult[0] == 1u, "an all-long tile gives 1");
    for (int i = 0; i < 64; ++i) len[i] = 0.0f;
    expect(bd_host_plan(&o, len.get(), 8, 8, mult.get(), &why) == RT_OK && mult[0] == 8u, "an all-zero tile gives target");
    o.max_mult = 3;
    expect(bd_host_plan(&o, len.get(), 8, 8, mult.get(), &why) == RT_OK && mult[0] == 3u, "... capped by max_mult");
    o.max_mult = 8;
    // exactly the quantile's count of pixels without history (16 of 64), then one fewer
    for (int i = 0; i < 64; ++i) len[i] = i < 16 ? 0.0f : 32.0f;
    expect(bd_host_plan(&o, len.get(), 8, 8, mult.get(), &why) == RT_OK && mult[0] == 8u, "the quantile's count of short pixels");
    len[15] = 32.0f;
    expect(bd_host_plan(&o, len.get(), 8, 8, mult.get(), &why) == RT_OK && mult[0] == 1u, "one fewer than the quantile");
    // the 16 shortest hold 5 frames: j* = 6, mult = 8 - 5 = 3
    for (int i = 0; i < 64; ++i) len[i] = i < 16 ? 5.0f : 32.0f;
    expect(bd_host_plan(&o, len.get(), 8, 8, mult.get(), &why) == RT_OK && mult[0] == 3u, "5 frames short of 8 gives 3");
    for (int i = 0; i < 64; ++i) len[i] = NAN;
    expect(bd_host_plan(&o, len.get(), 8, 8, mult.get(), &why) == RT_OK && mult[0] == 8u, "a NaN counts as short");
    *calls += 7;
  }
  // hostile lengths on sizes with partial tiles: the multipliers stay in range
  const int sizes[][2] = {{1, 1}, {9, 12}, {17, 33}, {40, 33}, {1, 65}, {65, 1}};   // rows x width
  for (const auto& sz : sizes)
    for (const int target : {1, 8, 32})
      for (const int q : {1, 16, 64})
        for (const int max_mult : {1, 4, 16}) {
          const int rows = sz[0], width = sz[1];
          const size_t n = static_cast<size_t>(rows) * width;
          const size_t nt = static_cast<size_t>((rows + 7) / 8) * ((width + 7) / 8);
          auto len = block(n);
          auto mult = ublock(nt);
          for (size_t i = 0; i < n; ++i) len[i] = draw(rng, 0.0f, 40.0f, 0.3f);
          const rt_budget_opts o{2, target, max_mult, q};
          const int rc = bd_host_plan(&o, len.get(), width, rows, mult.get(), &why);
          ++*calls;
          expect(rc == RT_OK, "a plan over hostile lengths");
          for (size_t t = 0; t < nt; ++t)
            expect(mult[t] >= 1u && mult[t] <= static_cast<uint32_t>(max_mult), "a multiplier outside 1..max_mult");
        }
  // refusals: nothing written
  {
    auto len = block(1);
    auto mult = ublock(1);
    len[0] = 0.0f;
    const rt_budget_opts bad[] = {{0, 8, 8, 16},  {1, 0, 8, 16},  {1, 33, 8, 16},       {1, 8, 0, 16},
                                  {1, 8, 17, 16}, {1, 8, 8, 0},   {1, 8, 8, 65},        {RT_MAX_SPP, 8, 8, 16},
                                  {-1, 8, 8, 16}, {1, -1, 8, 16}, {RT_MAX_SPP / 16 + 1, 8, 8, 16}};
    for (const rt_budget_opts& o : bad) {
      mult[0] = 77u;
      ++*calls;
      expect(bd_host_plan(&o, len.get(), 1, 1, mult.get(), &why) == RT_E_ARG && mult[0] == 77u && why, "bad options refused");
    }
    const rt_budget_opts ok{1, 8, 8, 16};
    mult[0] = 77u;
    expect(bd_host_plan(nullptr, len.get(), 1, 1, mult.get(), &why) == RT_E_ARG, "NULL options refused");
    expect(bd_host_plan(&ok, nullptr, 1, 1, mult.get(), &why) == RT_E_ARG, "NULL lengths refused");
    expect(bd_host_plan(&ok, len.get(), 1, 1, nullptr, &why) == RT_E_ARG, "NULL output refused");
    expect(bd_host_plan(&ok, len.get(), 0, 1, mult.get(), &why) == RT_E_ARG, "width 0 refused");
    expect(bd_host_plan(&ok, len.get(), 1, -1, mult.get(), &why) == RT_E_ARG && mult[0] == 77u, "rows < 0 refused");
    *calls += 5;
  }
}

}  // namespace

int main() {
  Rng rng{8642};
  long calls = 0, pixels = 0, with_history = 0, bad_len = 0;
  plan_cases(rng, &calls);

  // ---- the probe and the weighted step ----
  const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {9, 13}, {4, 64}, {17, 33}};   // rows x width
  constexpr int kBodies = 5;
  const uint32_t odd_mult[] = {0u, 1u, 2u, 8u, 16u, 17u, 0x80000000u, 0xffffffffu};
  for (const auto& sz : sizes) {
    const int rows = sz[0], width = sz[1];
    const size_t n = static_cast<size_t>(rows) * width;
    const size_t nt = static_cast<size_t>((rows + 7) / 8) * ((width + 7) / 8);
    for (const int row0 : {0, 5, 0x7fffffff - rows}) {
      const rt_camera cur = pinhole(width, rows, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
      const rt_camera prevs[] = {cur, pinhole(width, rows, 0.03f, -0.02f, 0.0f, 0.01f, 1.0f),
                                 pinhole(width, rows, 1.0f, 1.0f, 0.0f, 0x1p-31f, 1.0f)};
      for (const rt_camera& prev : prevs)
        for (const float p_odd : {0.0f, 0.3f, 1.0f})
          for (const float gamma : {1.0f, INFINITY})
            for (const bool with_ids : {false, true}) {
              auto half0 = block(3 * n), half1 = block(3 * n), feat = block(8 * n), a0 = block(3 * n), a1 = block(3 * n),
                   guide = block(4 * n), len = block(n), out0 = block(3 * n), out1 = block(3 * n), out_len = block(n),
                   motion = block(4 * kBodies), probe = block(n);
              auto mult = ublock(nt), mult_c = ublock(nt), ones = ublock(nt);
              std::unique_ptr<int32_t[]> ids(new int32_t[n]);
              for (size_t i = 0; i < 3 * n; ++i) {
                half0[i] = draw(rng, 0.0f, 2.0f, p_odd);
                half1[i] = draw(rng, 0.0f, 2.0f, p_odd);
                a0[i] = draw(rng, 0.0f, 2.0f, p_odd);
                a1[i] = draw(rng, 0.0f, 2.0f, p_odd);
              }
              for (size_t i = 0; i < n; ++i) {
                for (int c = 0; c < 8; ++c) feat[8 * i + c] = draw(rng, -1.0f, 1.0f, p_odd);
                if (p_odd == 0.0f) feat[8 * i + 3] = 0.0f, feat[8 * i + 4] = 0.6f, feat[8 * i + 5] = 0.8f;
                feat[8 * i + 6] = p_odd == 0.0f ? 9.0f + 0.01f * rng.uni() : draw(rng, 0.5f, 30.0f, 0.5f);
                for (int c = 0; c < 4; ++c) guide[4 * i + c] = p_odd > 0.0f ? draw(rng, 0.5f, 30.0f, p_odd) : feat[8 * i + 3 + c];
                len[i] = draw(rng, 0.0f, 40.0f, p_odd);
                ids[i] = static_cast<int32_t>(rng.next() % (kBodies + 6)) - 3;
              }
              for (size_t t = 0; t < nt; ++t) {
                mult[t] = odd_mult[rng.next() % (sizeof odd_mult / sizeof odd_mult[0])];
                mult_c[t] = mult[t] < 1u ? 1u : (mult[t] > 16u ? 16u : mult[t]);
                ones[t] = 1u;
              }
              for (int i = 0; i < 4 * kBodies; ++i) motion[i] = draw(rng, -0.05f, 0.05f, p_odd * 0.3f);
              rt_temporal_opts o = tp_default_opts();
              o.sigma_z = p_odd > 0.0f ? 3e38f : 0.1f;
              o.normal_min = p_odd > 0.0f ? -1.0f : 0.9f;
              const rt_temporal_clamp_opts k{2, gamma};
              const char* why = nullptr;
              const int32_t* idp = with_ids ? ids.get() : nullptr;
              // the probe
              int rc = tp_host_probe(&o, &cur, &prev, width, rows, row0, feat.get(), guide.get(), len.get(), idp,
                                     motion.get(), kBodies, probe.get(), &why);
              ++calls;
              expect(rc == RT_OK, "the probe");
              // the weighted step; its stored length is min(len + wt, max_history)
              rc = tp_host_step_budget(&o, &k, &cur, &prev, width, rows, row0, half0.get(), half1.get(), feat.get(),
                                       a0.get(), a1.get(), guide.get(), len.get(), idp, motion.get(), kBodies, mult.get(),
                                       out0.get(), out1.get(), out_len.get(), &why);
              ++calls;
              expect(rc == RT_OK, "the weighted step");
              const int gx = (width + 7) / 8;
              for (size_t i = 0; i < n; ++i) {
                ++pixels;
                const float wt = static_cast<float>(mult_c[(i / width / 8) * gx + (i % width) / 8]);
                const float sum = probe[i] + wt, mh = static_cast<float>(o.max_history);
                const float want = sum < mh ? sum : mh;   // dn_min's text
                // (a NaN length: accL of hostile history; the bits still agree)
                if (!same(&want, &out_len[i], 1)) ++bad_len;
                if (probe[i] > 0.0f) ++with_history;
              }
              // multipliers outside 1..16 behave as their clamped values
              auto c0 = block(3 * n), c1 = block(3 * n), cl = block(n);
              rc = tp_host_step_budget(&o, &k, &cur, &prev, width, rows, row0, half0.get(), half1.get(), feat.get(),
                                       a0.get(), a1.get(), guide.get(), len.get(), idp, motion.get(), kBodies, mult_c.get(),
                                       c0.get(), c1.get(), cl.get(), &why);
              ++calls;
              expect(rc == RT_OK && same(c0.get(), out0.get(), 3 * n) && same(c1.get(), out1.get(), 3 * n) &&
                         same(cl.get(), out_len.get(), n),
                     "multipliers outside 1..16 are clamped");
              // multipliers of one: the clamped step's bits
              rc = tp_host_step_budget(&o, &k, &cur, &prev, width, rows, row0, half0.get(), half1.get(), feat.get(),
                                       a0.get(), a1.get(), guide.get(), len.get(), idp, motion.get(), kBodies, ones.get(),
                                       out0.get(), out1.get(), out_len.get(), &why);
              const int rc2 = tp_host_step_clamp(&o, &k, &cur, &prev, width, rows, row0, half0.get(), half1.get(),
                                                 feat.get(), a0.get(), a1.get(), guide.get(), len.get(), idp, motion.get(),
                                                 kBodies, c0.get(), c1.get(), cl.get(), &why);
              calls += 2;
              expect(rc == RT_OK && rc2 == RT_OK && same(c0.get(), out0.get(), 3 * n) && same(c1.get(), out1.get(), 3 * n) &&
                         same(cl.get(), out_len.get(), n),
                     "multipliers of one give the clamped step");
            }
    }
  }
  // no previous camera: the probe is 0, the weighted step stores min(wt, max_history); refusals
  {
    auto half0 = block(3), half1 = block(3), feat = block(8), out0 = block(3), out1 = block(3), out_len = block(1);
    auto mult = ublock(1);
    for (int c = 0; c < 3; ++c) half0[c] = half1[c] = 0.5f;
    for (int c = 0; c < 8; ++c) feat[c] = NAN;
    const rt_camera cur = pinhole(1, 1, 0.0f, 0.0f, 0.0f, 0.01f, 1.0f);
    const char* why = nullptr;
    out_len[0] = 7.0f;
    int rc = tp_host_probe(nullptr, &cur, nullptr, 1, 1, 0, feat.get(), nullptr, nullptr, nullptr, nullptr, 0,
                           out_len.get(), &why);
    expect(rc == RT_OK && out_len[0] == 0.0f, "no previous camera: the probe is 0");
    mult[0] = 8u;
    rt_temporal_opts o = tp_default_opts();
    for (const int mh : {32, 4}) {
      o.max_history = mh;
      rc = tp_host_step_budget(&o, nullptr, &cur, nullptr, 1, 1, 0, half0.get(), half1.get(), feat.get(), nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, 0, mult.get(), out0.get(), out1.get(), out_len.get(),
                               &why);
      expect(rc == RT_OK && out_len[0] == (mh == 32 ? 8.0f : 4.0f) && out0[0] == 0.5f, "no history: N = min(wt, max_history)");
    }
    out_len[0] = 7.0f;
    rc = tp_host_step_budget(nullptr, nullptr, &cur, nullptr, 1, 1, 0, half0.get(), half1.get(), feat.get(), nullptr,
                             nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, out0.get(), out1.get(), out_len.get(),
                             &why);
    expect(rc == RT_E_ARG && out_len[0] == 7.0f, "a NULL mult is refused");
    const rt_temporal_clamp_opts bad{2, -1.0f};
    rc = tp_host_step_budget(nullptr, &bad, &cur, nullptr, 1, 1, 0, half0.get(), half1.get(), feat.get(), nullptr, nullptr,
                             nullptr, nullptr, nullptr, nullptr, 0, mult.get(), out0.get(), out1.get(), out_len.get(), &why);
    expect(rc == RT_E_ARG && out_len[0] == 7.0f, "a bad gamma is refused");
    rc = tp_host_probe(nullptr, &cur, nullptr, 1, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, out_len.get(), &why);
    expect(rc == RT_E_ARG && out_len[0] == 7.0f, "a NULL feat is refused");
    rc = tp_host_probe(nullptr, &cur, &cur, 1, 1, 0, feat.get(), nullptr, nullptr, nullptr, nullptr, 0, out_len.get(), &why);
    expect(rc == RT_E_ARG && out_len[0] == 7.0f, "a previous camera without history is refused");
    calls += 7;
  }
  std::printf("{\"calls\": %ld, \"bad\": %ld, \"pixels\": %ld, \"with_history\": %ld, \"bad_len\": %ld}\n", calls, g_bad,
              pixels, with_history, bad_len);
  return g_bad == 0 && bad_len == 0 && with_history > 0 ? 0 : 1;
}
