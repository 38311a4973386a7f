// upsample_check — guided upsampling (csrc/upsample.h: up_host, the body of
// rt_upsample_host, and up_pixel, the text upsample_kernel runs) built for the
// host under the sanitizers, over inputs rt.h leaves unspecified: the numbers
// may be anything, the indices may not.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all -static-libasan -static-libubsan tools/upsample_check.cpp
//
// Every array is a heap block of exactly its size, so a tap outside the coarse
// image is a report.  Inputs: colours, albedos, normals, depths and coverages
// drawn from ordinary values mixed with NaN, +-inf, 0, negatives, denormals,
// 1e30 and 3e38; every image from 1 x 1 to 9 x 13 at every scale, one image
// and two, the default options and the ranges' ends.  With ordinary inputs
// every output must be finite; the axis taps are checked against rt.h's
// integers over the first 4096 coordinates and at the top of the range.  One
// JSON line; exit status 0 when every call returned what it should.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>

#include "../include/rt.h"
#include "../raytracing-clj_amd/csrc/upsample.h"

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

const float kOdd[] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, -1.0f, -4.0f, 1e-42f, 1e30f, -1e30f, 3e38f, -3e38f};

// an ordinary value in [lo, hi), or with probability p one of kOdd
float draw(Rng& r, float lo, float hi, float p) {
  if (r.uni() < p) return kOdd[r.next() % (sizeof kOdd / sizeof kOdd[0])];
  return lo + (hi - lo) * r.uni();
}

// exactly n floats on the heap (no slack behind them)
std::unique_ptr<float[]> block(size_t n) { return std::unique_ptr<float[]>(new float[n]); }

void fill_feat(Rng& rng, float* f, size_t n, float p_odd) {
  for (size_t i = 0; i < n; ++i) {
    for (int c = 0; c < 3; ++c) f[8 * i + c] = draw(rng, 0.0f, 1.0f, p_odd);
    for (int c = 3; c < 6; ++c) f[8 * i + c] = draw(rng, -1.0f, 1.0f, p_odd);
    f[8 * i + 6] = draw(rng, 0.5f, 30.0f, p_odd > 0.0f ? 0.5f : 0.0f);   // depths: NaN, <= 0, +-inf among them
    f[8 * i + 7] = draw(rng, 0.0f, 1.0f, p_odd);
    if (p_odd == 0.0f && rng.uni() < 0.2f) {   // a sky pixel as rt_feat_resolve writes it
      for (int c = 0; c < 6; ++c) f[8 * i + c] = 0.0f;
      f[8 * i + 6] = INFINITY;
      f[8 * i + 7] = 0.0f;
    }
  }
}

}  // namespace

int main() {
  Rng rng{54321};
  long calls = 0, bad_status = 0, pixels = 0, not_finite = 0, bad_axis = 0, fallbacks = 0;
  // step 1 against its definition in 64-bit integers
  for (int s = kUpMinScale; s <= kUpMaxScale; ++s)
    for (int k = 0; k < 8192; ++k) {
      const int x = k < 4096 ? k : 0x7fffffff - (k - 4096);
      const int64_t u = 2 * static_cast<int64_t>(x) + 1 - s;
      const int64_t X0 = u >= 0 ? u / (2 * s) : -((-u + 2 * s - 1) / (2 * s));
      const int64_t a = u - 2 * s * X0;
      int got;
      float b0, b1;
      up_axis(x, s, &got, &b0, &b1);
      if (got != X0 || a < 0 || a >= 2 * s || b0 != static_cast<float>(2 * s - a) / static_cast<float>(2 * s) ||
          b1 != static_cast<float>(a) / static_cast<float>(2 * s))
        ++bad_axis;
    }
  for (int rows = 1; rows <= 9; ++rows)
    for (int width = 1; width <= 13; ++width)
      for (int s = kUpMinScale; s <= kUpMaxScale; ++s)
        for (const float p_odd : {0.0f, 0.3f, 1.0f})
          for (const int two : {0, 1})
            for (const int variant : {0, 1, 2}) {
              const size_t n = static_cast<size_t>(rows) * width;
              const size_t nc = static_cast<size_t>(up_coarse(rows, s)) * up_coarse(width, s);
              auto half0 = block(3 * nc), half1 = block(3 * nc), fc = block(8 * nc), ff = block(8 * n),
                   out0 = block(3 * n), out1 = block(3 * n);
              for (size_t i = 0; i < 3 * nc; ++i) {
                half0[i] = draw(rng, 0.0f, 2.0f, p_odd);
                half1[i] = draw(rng, 0.0f, 2.0f, p_odd);
              }
              fill_feat(rng, fc.get(), nc, p_odd);
              fill_feat(rng, ff.get(), n, p_odd);
              rt_upsample_opts o = up_default_opts();
              o.scale = s;
              if (variant == 1) o.normal_pow2 = 8, o.sigma_z = 1e-38f;
              if (variant == 2) o.normal_pow2 = 5, o.sigma_z = 3e38f;
              const char* why = nullptr;
              const int rc = up_host(&o, half0.get(), two ? half1.get() : nullptr, fc.get(), ff.get(), width, rows,
                                     out0.get(), two ? out1.get() : nullptr, &why);
              ++calls;
              if (rc != RT_OK) {
                ++bad_status;
                continue;
              }
              pixels += static_cast<long>(n);
              if (p_odd == 0.0f)
                for (size_t i = 0; i < 3 * n; ++i)
                  if (!std::isfinite(out0[i]) || (two && !std::isfinite(out1[i]))) ++not_finite;
              if (p_odd == 0.0f && variant == 1)   // (sigma_z of 1e-38 and sky against surface: most pixels fall back)
                for (int y = 0; y < rows; ++y)
                  for (int x = 0; x < width; ++x) {
                    // the guided weights of this pixel, to count the fallback's share
                    int X0, Y0;
                    float bx[2], by[2], wsum = 0.0f;
                    up_axis(x, s, &X0, &bx[0], &bx[1]);
                    up_axis(y, s, &Y0, &by[0], &by[1]);
                    const float* fp = ff.get() + 8 * (static_cast<size_t>(y) * width + x);
                    for (int ty = 0; ty < 2; ++ty)
                      for (int tx = 0; tx < 2; ++tx) {
                        const int X = X0 + tx, Y = Y0 + ty;
                        if (X < 0 || X >= up_coarse(width, s) || Y < 0 || Y >= up_coarse(rows, s)) continue;
                        const float* fq = fc.get() + 8 * (static_cast<size_t>(Y) * up_coarse(width, s) + X);
                        float wn, wz;
                        up_guide_weight(DnGuide{fp[3], fp[4], fp[5], fp[6]}, 1.0f - fp[7],
                                        DnGuide{fq[3], fq[4], fq[5], fq[6]}, 1.0f - fq[7], s, o.normal_pow2, o.sigma_z,
                                        &wn, &wz);
                        wsum += ((by[ty] * bx[tx]) * wn) * wz;
                      }
                    if (!(wsum >= 0x1p-10f)) ++fallbacks;
                  }
            }
  // the refusals: options, sizes, pointers, overlaps
  {
    auto h = block(3), fc = block(8), ff = block(8), o0 = block(3), o1 = block(3);
    for (int c = 0; c < 3; ++c) h[c] = 1.0f;
    for (int c = 0; c < 8; ++c) fc[c] = ff[c] = 0.5f;
    const char* why = nullptr;
    rt_upsample_opts o = up_default_opts();
    auto refused = [&](int rc) {
      ++calls;
      if (rc != RT_E_ARG || !why) ++bad_status;
    };
    o.scale = 1;
    refused(up_host(&o, h.get(), nullptr, fc.get(), ff.get(), 1, 1, o0.get(), nullptr, &why));
    o.scale = 5;
    refused(up_host(&o, h.get(), nullptr, fc.get(), ff.get(), 1, 1, o0.get(), nullptr, &why));
    o = up_default_opts();
    o.sigma_z = NAN;
    refused(up_host(&o, h.get(), nullptr, fc.get(), ff.get(), 1, 1, o0.get(), nullptr, &why));
    o = up_default_opts();
    o.normal_pow2 = 9;
    refused(up_host(&o, h.get(), nullptr, fc.get(), ff.get(), 1, 1, o0.get(), nullptr, &why));
    refused(up_host(nullptr, nullptr, nullptr, fc.get(), ff.get(), 1, 1, o0.get(), nullptr, &why));
    refused(up_host(nullptr, h.get(), h.get(), fc.get(), ff.get(), 1, 1, o0.get(), nullptr, &why));
    refused(up_host(nullptr, h.get(), nullptr, fc.get(), ff.get(), 1, 1, o0.get(), o1.get(), &why));
    refused(up_host(nullptr, h.get(), nullptr, fc.get(), ff.get(), 0, 1, o0.get(), nullptr, &why));
    refused(up_host(nullptr, h.get(), nullptr, fc.get(), ff.get(), 65536, 32768, o0.get(), nullptr, &why));
    refused(up_host(nullptr, h.get(), nullptr, fc.get(), ff.get(), 1, 1, h.get(), nullptr, &why));
    refused(up_host(nullptr, h.get(), h.get(), fc.get(), ff.get(), 1, 1, o0.get(), o0.get(), &why));
  }
  std::printf("{\"calls\": %ld, \"bad_status\": %ld, \"pixels\": %ld, \"not_finite\": %ld, \"bad_axis\": %ld, "
              "\"fallbacks\": %ld}\n",
              calls, bad_status, pixels, not_finite, bad_axis, fallbacks);
  return bad_status == 0 && not_finite == 0 && bad_axis == 0 && fallbacks > 0 ? 0 : 1;
}
