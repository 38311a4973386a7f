// denoise.h — the feature-guided denoiser (rt_denoise, include/rt.h): an
// edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over
// albedo-demodulated colour, guided by rt_feat_resolve's normal, depth and
// coverage, its colour edge-stop scaled by the variance two half-frames give
// (the SVGF manner).
//
// Replaces nothing the reference computes: it consumes what compute-pixel's
// loop (src/raytracing.clj:141-155) leaves in rt_accum / rt_adapt / rt_feat.
//
// Two parts, as first_hit.h.
//  1. The definition as plain inline functions that compile for the device
//     (the kernels below) and for the host (rt_denoise_host, rt_host.cpp):
//     the prep of one pixel, the weight of one tap, one pixel of one level.
//     One text for both: every line is one fp32 operation rounded once, in
//     rt.h's order (the library is built with -ffp-contract=off); / and sqrt
//     are IEEE on either side (fp_rn.h's sqrt_rn / rcp_rn on the device,
//     which give the same bits).  A pixel reads its neighbours through a
//     `Src` -- four accessors over the packed arrays -- so a kernel may serve
//     them from wherever it staged them.
//  2. The device kernels (under __HIPCC__ and RT_DENOISE_KERNEL): one thread
//     per output pixel, no atomics, no scratch; the bits cannot depend on the
//     launch shape.
//
// Packed arrays (rows x width each): texel (m_r, m_g, m_b, var), 16 bytes,
// ping-ponged between levels; guide (n_x, n_y, n_z, z), 16 bytes, and
// omc = 1 - cov, 4 bytes, written once by the prep.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/rt.h"

#if defined(__HIPCC__)
#include "fp_rn.h"
#define RT_DN_FN __host__ __device__ __forceinline__
#else
#define RT_DN_FN inline
#endif

namespace rtclj {

struct alignas(16) DnTexel {
  float r, g, b, var;
};
struct alignas(16) DnGuide {
  float nx, ny, nz, z;
};

constexpr int kDnMaxLevels = 8, kDnMaxPow2 = 8;

// rt.h's defaults
RT_DN_FN rt_denoise_opts dn_default_opts() {
  rt_denoise_opts o;
  o.levels = 5;
  o.normal_pow2 = 5;
  o.sigma_c = 4.0f;
  o.sigma_z = 0.05f;
  return o;
}
// nullptr, or which rule of rt.h's table the options break
inline const char* dn_opts_error(const rt_denoise_opts& o) {
  if (o.levels < 1 || o.levels > kDnMaxLevels) return "levels outside 1..8";
  if (o.normal_pow2 < 0 || o.normal_pow2 > kDnMaxPow2) return "normal_pow2 outside 0..8";
  if (!(o.sigma_c > 0.0f) || !(o.sigma_c < INFINITY)) return "sigma_c is not finite and > 0";
  if (!(o.sigma_z > 0.0f) || !(o.sigma_z < INFINITY)) return "sigma_z is not finite and > 0";
  return nullptr;
}

// correctly rounded sqrt and reciprocal: the same bits on host and device
RT_DN_FN float dn_sqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}
RT_DN_FN float dn_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return rcp_rn(x);
#else
  return 1.0f / x;
#endif
}
RT_DN_FN float dn_max(float a, float b) { return a > b ? a : b; }
RT_DN_FN float dn_min(float a, float b) { return a < b ? a : b; }
RT_DN_FN float dn_abs(float a) { return a < 0.0f ? -a : a; }

RT_DN_FN float dn_lum(float r, float g, float b) { return (r * 0.2126f + g * 0.7152f) + b * 0.0722f; }

// the albedo a colour is divided by and multiplied back with
RT_DN_FN float dn_albedo(float a) { return dn_max(a, 0x1p-10f); }

// Prep of one pixel: half0, half1 (3 floats each) and feat (8 floats) ->
// texel, guide and 1 - cov.
RT_DN_FN void dn_prep(const float* h0, const float* h1, const float* feat, DnTexel* t, DnGuide* g, float* omc) {
  float ia[3], ib[3], m[3];
  for (int c = 0; c < 3; ++c) {
    const float alb = dn_albedo(feat[c]);
    ia[c] = h0[c] / alb;
    ib[c] = h1[c] / alb;
    m[c] = 0.5f * (ia[c] + ib[c]);
  }
  const float d = dn_lum(ia[0], ia[1], ia[2]) - dn_lum(ib[0], ib[1], ib[2]);
  t->r = m[0];
  t->g = m[1];
  t->b = m[2];
  t->var = 0.25f * d * d;
  g->nx = feat[3];
  g->ny = feat[4];
  g->nz = feat[5];
  g->z = feat[6];
  *omc = 1.0f - feat[7];
}

// What a level needs of the centre pixel, once.
struct DnCentre {
  DnGuide g;
  float omc, lum, sd;
};

// The weight of the tap at q (not the centre) whose kernel weight is k and
// whose distance in pixels is dist = s * max(|dx|, |dy|).
RT_DN_FN float dn_tap_weight(const DnCentre& p, const DnGuide& gq, float omc_q, float lum_q, float k, int dist,
                             int normal_pow2, float sigma_z) {
  const float dot = ((p.g.nx * gq.nx + p.g.ny * gq.ny) + p.g.nz * gq.nz) + p.omc * omc_q;
  float wn = dn_min(1.0f, dn_max(0.0f, dot));
  for (int j = 0; j < normal_pow2; ++j) wn = wn * wn;
  float wz;
  const bool pinf = p.g.z == INFINITY, qinf = gq.z == INFINITY;
  if (pinf && qinf) {
    wz = 1.0f;
  } else if (pinf || qinf) {
    wz = 0.0f;
  } else {
    const float r = dn_abs(p.g.z - gq.z) / ((sigma_z * static_cast<float>(dist)) * dn_min(p.g.z, gq.z));
    wz = dn_rcp(1.0f + r * r);
  }
  const float rc = dn_abs(p.lum - lum_q) / p.sd;
  const float wc = dn_rcp(1.0f + rc * rc);
  return ((k * wn) * wz) * wc;
}

// One pixel (x, y) of the level with step s: the new texel.  Src:
//   DnTexel texel(int x, int y), float var(int x, int y),
//   DnGuide guide(int x, int y), float omc(int x, int y)
// called for pixels inside the width x rows image only.
template <class Src>
RT_DN_FN DnTexel dn_level_pixel(const Src& src, int x, int y, int width, int rows, int s, int normal_pow2,
                                float sigma_c, float sigma_z) {
  const DnTexel tp = src.texel(x, y);
  // the variance's 3 x 3 binomial mean at step 1
  float num = 0.0f, den = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -1; dy <= 1; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
      const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
      const float vq = (dx == 0 && dy == 0) ? tp.var : src.var(qx, qy);
      num += k * vq;
      den += k;
    }
  }
  DnCentre p;
  p.g = src.guide(x, y);
  p.omc = src.omc(x, y);
  p.lum = dn_lum(tp.r, tp.g, tp.b);
  p.sd = dn_sqrt(num / den) * sigma_c + 1e-6f;
  float acc[3] = {0.0f, 0.0f, 0.0f}, accv = 0.0f, wsum = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -2; dy <= 2; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -2; dx <= 2; ++dx) {
      const int ay = dy < 0 ? -dy : dy, ax = dx < 0 ? -dx : dx;
      const float hy = ay == 0 ? 0.375f : ay == 1 ? 0.25f : 0.0625f;
      const float hx = ax == 0 ? 0.375f : ax == 1 ? 0.25f : 0.0625f;
      const float k = hy * hx;
      float w;
      DnTexel tq;
      if (dx == 0 && dy == 0) {
        tq = tp;
        w = k;
      } else {
        // (|s * d| <= 256: no overflow for any int x, y inside the image)
        const int qx = x + s * dx, qy = y + s * dy;
        if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
        tq = src.texel(qx, qy);
        w = dn_tap_weight(p, src.guide(qx, qy), src.omc(qx, qy), dn_lum(tq.r, tq.g, tq.b), k, s * (ax > ay ? ax : ay),
                          normal_pow2, sigma_z);
      }
      acc[0] += w * tq.r;
      acc[1] += w * tq.g;
      acc[2] += w * tq.b;
      accv += (w * w) * tq.var;
      wsum += w;
    }
  }
  DnTexel o;
  o.r = acc[0] / wsum;
  o.g = acc[1] / wsum;
  o.b = acc[2] / wsum;
  o.var = accv / (wsum * wsum);
  return o;
}

// The packed arrays read in place (the host; the device's direct loads).
struct DnArrays {
  const DnTexel* t;
  const DnGuide* g;
  const float* o;
  int width;
  RT_DN_FN size_t at(int x, int y) const { return static_cast<size_t>(y) * width + x; }
  RT_DN_FN DnTexel texel(int x, int y) const { return t[at(x, y)]; }
  RT_DN_FN float var(int x, int y) const { return t[at(x, y)].var; }
  RT_DN_FN DnGuide guide(int x, int y) const { return g[at(x, y)]; }
  RT_DN_FN float omc(int x, int y) const { return o[at(x, y)]; }
};

// Output of one pixel: the last level's colour times the albedo again.
RT_DN_FN void dn_finish(const DnTexel& t, const float* feat, float* out) {
  out[0] = t.r * dn_albedo(feat[0]);
  out[1] = t.g * dn_albedo(feat[1]);
  out[2] = t.b * dn_albedo(feat[2]);
}

// A workgroup of the image kernels (here, temporal.h, body_ids.h) is kDnBx x
// kDnBy pixels, a wave one row of 64: a tap of a wave is 64 consecutive
// 16-byte words, 1 KiB per load instruction.
constexpr int kDnBx = 64, kDnBy = 4;

#if defined(__HIPCC__) && defined(RT_DENOISE_KERNEL)
// ------------------------------------------------------------ the kernels ----

// The prep: a thread per pixel, grid-stride.  The caller's arrays are read as
// single floats (they need no more than a float's alignment), the packed
// arrays written as 16-byte words.
__global__ __launch_bounds__(256) void denoise_prep_kernel(const float* __restrict__ half0,
                                                            const float* __restrict__ half1,
                                                            const float* __restrict__ feat, size_t n_px,
                                                            DnTexel* __restrict__ texel, DnGuide* __restrict__ guide,
                                                            float* __restrict__ omc) {
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n_px; i += stride) {
    float h0[3], h1[3], f[RT_FEAT_CHANNELS];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      h0[c] = half0[i * 3 + c];
      h1[c] = half1[i * 3 + c];
    }
#pragma unroll
    for (int c = 0; c < RT_FEAT_CHANNELS; ++c) f[c] = feat[i * RT_FEAT_CHANNELS + c];
    DnTexel t;
    DnGuide g;
    float o;
    dn_prep(h0, h1, f, &t, &g, &o);
    texel[i] = t;
    guide[i] = g;
    omc[i] = o;
  }
}

// One level at any step (the launch code runs it from step 4 on): thread
// (x, y) owns output pixel (x, y) and reads its taps from the packed arrays
// directly (the 25 taps of neighbouring pixels meet in the vector L1 and the
// L2).  LAST: the level's colour is not stored as a texel
// but re-modulated into `out` (rows x width x 3 floats), the finish folded in.
template <bool LAST>
__global__ __launch_bounds__(kDnBx* kDnBy) void denoise_level_kernel(const DnTexel* __restrict__ src,
                                                                     const DnGuide* __restrict__ guide,
                                                                     const float* __restrict__ omc, int width, int rows,
                                                                     int s, int normal_pow2, float sigma_c,
                                                                     float sigma_z, DnTexel* __restrict__ dst,
                                                                     const float* __restrict__ feat,
                                                                     float* __restrict__ out) {
  const int x = static_cast<int>(blockIdx.x) * kDnBx + static_cast<int>(threadIdx.x);
  const int y = static_cast<int>(blockIdx.y) * kDnBy + static_cast<int>(threadIdx.y);
  if (x >= width || y >= rows) return;
  const DnArrays a{src, guide, omc, width};
  const DnTexel t = dn_level_pixel(a, x, y, width, rows, s, normal_pow2, sigma_c, sigma_z);
  const size_t i = a.at(x, y);
  if (LAST) {
    float f[3], o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = feat[i * RT_FEAT_CHANNELS + c];
    dn_finish(t, f, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = o[c];
  } else {
    dst[i] = t;
  }
}
// The levels whose halo is small (S = 1, 2): the workgroup first stages its
// pixels and a halo of 2 S around them -- texel, guide and 1 - cov, 36 bytes a
// pixel: 19,584 bytes at S = 1, 31,104 at S = 2 -- in LDS, and every tap is a
// ds_read_b128 pair and a ds_read_b32.  Words of the tile that lie outside the
// image are never written and never read (a tap outside the image is skipped
// before its load).  C1's frame: level 0 48 us against the direct kernel's 56,
// level 1 54 against 57; from S = 4 on the tile would pass
// 64 KiB for no gain (the levels are VALU-bound) and the direct kernel runs.
template <int S>
struct DnTile {
  static constexpr int kHalo = 2 * S, kW = kDnBx + 2 * kHalo, kH = kDnBy + 2 * kHalo, kN = kW * kH;
  const DnTexel* t;
  const DnGuide* g;
  const float* o;
  int x0, y0;   // the image position of the tile's first word
  __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * kW + (x - x0); }
  __device__ __forceinline__ DnTexel texel(int x, int y) const { return t[at(x, y)]; }
  __device__ __forceinline__ float var(int x, int y) const { return t[at(x, y)].var; }
  __device__ __forceinline__ DnGuide guide(int x, int y) const { return g[at(x, y)]; }
  __device__ __forceinline__ float omc(int x, int y) const { return o[at(x, y)]; }
};
template <int S, bool LAST>
__global__ __launch_bounds__(kDnBx* kDnBy) void denoise_level_lds_kernel(
    const DnTexel* __restrict__ src, const DnGuide* __restrict__ guide, const float* __restrict__ omc, int width,
    int rows, int normal_pow2, float sigma_c, float sigma_z, DnTexel* __restrict__ dst,
    const float* __restrict__ feat, float* __restrict__ out) {
  using T = DnTile<S>;
  __shared__ DnTexel s_t[T::kN];
  __shared__ DnGuide s_g[T::kN];
  __shared__ float s_o[T::kN];
  const int x0 = static_cast<int>(blockIdx.x) * kDnBx - T::kHalo, y0 = static_cast<int>(blockIdx.y) * kDnBy - T::kHalo;
  for (int i = static_cast<int>(threadIdx.y) * kDnBx + static_cast<int>(threadIdx.x); i < T::kN; i += kDnBx * kDnBy) {
    const int ly = i / T::kW, gx = x0 + (i - ly * T::kW), gy = y0 + ly;
    if (gx >= 0 && gx < width && gy >= 0 && gy < rows) {
      const size_t j = static_cast<size_t>(gy) * width + gx;
      s_t[i] = src[j];
      s_g[i] = guide[j];
      s_o[i] = omc[j];
    }
  }
  __syncthreads();
  const int x = x0 + T::kHalo + static_cast<int>(threadIdx.x), y = y0 + T::kHalo + static_cast<int>(threadIdx.y);
  if (x >= width || y >= rows) return;
  const T tile{s_t, s_g, s_o, x0, y0};
  const DnTexel t = dn_level_pixel(tile, x, y, width, rows, S, normal_pow2, sigma_c, sigma_z);
  const size_t i = static_cast<size_t>(y) * width + x;
  if (LAST) {
    float f[3], o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = feat[i * RT_FEAT_CHANNELS + c];
    dn_finish(t, f, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = o[c];
  } else {
    dst[i] = t;
  }
}
#endif  // __HIPCC__ && RT_DENOISE_KERNEL

}  // namespace rtclj
