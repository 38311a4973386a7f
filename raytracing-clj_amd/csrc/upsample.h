// upsample.h — guided upsampling (rt_upsample, include/rt.h): two half-frames
// traced on a grid of scale x scale pixel blocks (rt_camera_coarsen's camera)
// brought up to the full size through the full-size first-hit features, a
// joint bilateral upsampling (Kopf et al. 2007) of albedo-demodulated colour
// whose weights are rt_denoise's normal, coverage and depth terms.
//
// Replaces nothing the reference computes: it consumes what compute-pixel's
// loop (src/raytracing.clj:141-155) leaves in rt_accum and rt_feat for two
// cameras, the frame's and the coarsened one (raytracing.clj:129-135).
//
// Two parts, as denoise.h.
//  1. The definition as plain inline functions that compile for the device
//     (the kernel below) and for the host (up_host, the body of
//     rt_upsample_host, and what tools/upsample_check.cpp runs under the
//     sanitizers): a pixel's taps along one axis, the weight of one tap, one
//     fine pixel.  One text for both: every line is one fp32 operation rounded
//     once, in rt.h's order; / is IEEE on either side.  A pixel reads its
//     coarse taps through a `Src` -- one accessor that gives a coarse pixel's
//     two irradiances and its guides -- so the kernel may serve them from LDS.
//  2. The device kernel (under __HIPCC__ and RT_UPSAMPLE_KERNEL): one thread
//     per fine pixel, no atomics, no scratch; the bits cannot depend on the
//     launch shape.
#pragma once
#include <cmath>
#include <cstdint>

#include "denoise.h"

namespace rtclj {

constexpr int kUpMinScale = 2, kUpMaxScale = 4;

// rt.h's defaults
RT_DN_FN rt_upsample_opts up_default_opts() {
  rt_upsample_opts o;
  o.scale = 2;
  o.normal_pow2 = 0;
  o.sigma_z = 0.05f;
  return o;
}
// nullptr, or which rule of rt.h's table the options break
inline const char* up_opts_error(const rt_upsample_opts& o) {
  if (o.scale < kUpMinScale || o.scale > kUpMaxScale) return "scale outside 2..4";
  if (o.normal_pow2 < 0 || o.normal_pow2 > kDnMaxPow2) return "normal_pow2 outside 0..8";
  if (!(o.sigma_z > 0.0f) || !(o.sigma_z < INFINITY)) return "sigma_z is not finite and > 0";
  return nullptr;
}
inline const char* up_shape_error(int width, int rows) {
  if (width <= 0 || rows <= 0 || static_cast<int64_t>(width) * rows > 0x7fffffffll) return "bad width/rows";
  return nullptr;
}
// the coarse image's extent along an axis of n fine pixels
RT_DN_FN int up_coarse(int n, int s) { return (n - 1) / s + 1; }

inline bool up_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

// Step 1 along one axis: fine coordinate x (0 <= x < 2^31) at scale s -> the
// first tap X0 (-1 in the first columns) and the two bilinear weights.
// u = 2 x + 1 - s is taken in unsigned 32 bits (2 x + 1 < 2^32); u < 0 only
// where 2 x + 1 < s, and then floor(u / 2 s) = -1 as u > -2 s.
RT_DN_FN void up_axis(int x, int s, int* X0, float* b0, float* b1) {
  const uint32_t t = 2u * static_cast<uint32_t>(x) + 1u, us = static_cast<uint32_t>(s), d = 2u * us;
  int a;
  if (t < us) {
    *X0 = -1;
    a = static_cast<int>((t + d) - us);
  } else {
    const uint32_t u = t - us, q = u / d;
    *X0 = static_cast<int>(q);
    a = static_cast<int>(u - d * q);
  }
  const float fd = static_cast<float>(static_cast<int>(d));
  *b0 = static_cast<float>(static_cast<int>(d) - a) / fd;
  *b1 = static_cast<float>(a) / fd;
}

// What a tap needs of a coarse pixel: both halves' irradiance (step 5) and
// the five guide floats.
struct UpCoarse {
  float i0[3], i1[3];
  DnGuide g;
  float omc;
};
// Step 5 and step 3's q of one coarse pixel: h0, h1 (3 floats each; h1 may be
// nullptr: one image) and its 8 feature floats.
RT_DN_FN UpCoarse up_coarse_pixel(const float* h0, const float* h1, const float* feat) {
  UpCoarse q;
  for (int c = 0; c < 3; ++c) {
    const float alb = dn_albedo(feat[c]);
    q.i0[c] = h0[c] / alb;
    q.i1[c] = h1 ? h1[c] / alb : 0.0f;
  }
  q.g.nx = feat[3];
  q.g.ny = feat[4];
  q.g.nz = feat[5];
  q.g.z = feat[6];
  q.omc = 1.0f - feat[7];
  return q;
}

// Step 4 without the bilinear factor: wn and wz of fine pixel p against coarse
// pixel q (dn_tap_weight's normal and depth terms with dist = s).
RT_DN_FN void up_guide_weight(const DnGuide& gp, float omc_p, const DnGuide& gq, float omc_q, int s, int normal_pow2,
                              float sigma_z, float* wn_out, float* wz_out) {
  const float dot = ((gp.nx * gq.nx + gp.ny * gq.ny) + gp.nz * gq.nz) + omc_p * omc_q;
  float wn = dn_min(1.0f, dn_max(0.0f, dot));
  for (int j = 0; j < normal_pow2; ++j) wn = wn * wn;
  float wz;
  const bool pinf = gp.z == INFINITY, qinf = gq.z == INFINITY;
  if (pinf && qinf) {
    wz = 1.0f;
  } else if (pinf || qinf) {
    wz = 0.0f;
  } else {
    const float r = dn_abs(gp.z - gq.z) / ((sigma_z * static_cast<float>(s)) * dn_min(gp.z, gq.z));
    wz = dn_rcp(1.0f + r * r);
  }
  *wn_out = wn;
  *wz_out = wz;
}

// One fine pixel (x, y) of the width x rows image: o0 and, with TWO, o1 (3
// floats each).  fp: the pixel's 8 feature floats.  cw x ch: the coarse image.
// Src: UpCoarse tap(int X, int Y), called for coarse pixels inside the coarse
// image only.  The guided sums (step 6) and the fallback's (step 7) are kept
// side by side -- the same operations in the same order as a second pass --
// so that every tap is fetched once.
template <bool TWO, class Src>
RT_DN_FN void up_pixel(const Src& src, int x, int y, int s, int cw, int ch, int normal_pow2, float sigma_z,
                       const float* fp, float* o0, float* o1) {
  int X0, Y0;
  float bx[2], by[2];
  up_axis(x, s, &X0, &bx[0], &bx[1]);
  up_axis(y, s, &Y0, &by[0], &by[1]);
  const DnGuide gp{fp[3], fp[4], fp[5], fp[6]};
  const float omc_p = 1.0f - fp[7];
  float acc0[3] = {0.0f, 0.0f, 0.0f}, acc1[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
  float fb0[3] = {0.0f, 0.0f, 0.0f}, fb1[3] = {0.0f, 0.0f, 0.0f}, bsum = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int ty = 0; ty < 2; ++ty) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int tx = 0; tx < 2; ++tx) {
      const int X = X0 + tx, Y = Y0 + ty;
      if (X < 0 || X >= cw || Y < 0 || Y >= ch) continue;
      const float b = by[ty] * bx[tx];
      const UpCoarse q = src.tap(X, Y);
      float wn, wz;
      up_guide_weight(gp, omc_p, q.g, q.omc, s, normal_pow2, sigma_z, &wn, &wz);
      const float w = (b * wn) * wz;
      for (int c = 0; c < 3; ++c) {
        acc0[c] += w * q.i0[c];
        fb0[c] += b * q.i0[c];
        if (TWO) {
          acc1[c] += w * q.i1[c];
          fb1[c] += b * q.i1[c];
        }
      }
      wsum += w;
      bsum += b;
    }
  }
  const bool fallback = !(wsum >= 0x1p-10f);
  const float den = fallback ? bsum : wsum;
  for (int c = 0; c < 3; ++c) {
    const float alb = dn_albedo(fp[c]);
    o0[c] = ((fallback ? fb0[c] : acc0[c]) / den) * alb;
    if (TWO) o1[c] = ((fallback ? fb1[c] : acc1[c]) / den) * alb;
  }
}

// The caller's coarse arrays read in place (the host).
struct UpPlain {
  const float *h0, *h1, *feat;
  int cw;
  UpCoarse tap(int X, int Y) const {
    const size_t j = static_cast<size_t>(Y) * cw + X;
    return up_coarse_pixel(h0 + 3 * j, h1 ? h1 + 3 * j : nullptr, feat + RT_FEAT_CHANNELS * j);
  }
};

// What rt_upsample and rt_upsample_host ask of their arguments (rt.h), or
// nullptr: the pointers, the options, the sizes, the outputs against the
// inputs and each other.
inline const char* up_args_error(const rt_upsample_opts& opt, const float* half0, const float* half1,
                                 const float* feat_coarse, const float* feat, int width, int rows, const float* out0,
                                 const float* out1) {
  if (!half0 || !feat_coarse || !feat || !out0) return "NULL argument";
  if ((half1 == nullptr) != (out1 == nullptr)) return "half1 and out1 must both be given or both be NULL";
  if (const char* why = up_opts_error(opt)) return why;
  if (const char* why = up_shape_error(width, rows)) return why;
  const size_t fb = sizeof(float), n_px = static_cast<size_t>(width) * rows;
  const size_t n_c = static_cast<size_t>(up_coarse(width, opt.scale)) * up_coarse(rows, opt.scale);
  const void* ins[4] = {half0, half1, feat_coarse, feat};
  const size_t in_b[4] = {n_c * 3 * fb, n_c * 3 * fb, n_c * RT_FEAT_CHANNELS * fb, n_px * RT_FEAT_CHANNELS * fb};
  const void* outs[2] = {out0, out1};
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 4; ++b)
      if (up_overlap(outs[a], n_px * 3 * fb, ins[b], in_b[b])) return "an output overlaps an input";
  if (up_overlap(out0, n_px * 3 * fb, out1, n_px * 3 * fb)) return "the outputs overlap";
  return nullptr;
}

// rt_upsample_host (rt.h): the checks, then every pixel.  0, or RT_E_ARG with
// *why set.
inline int up_host(const rt_upsample_opts* o, const float* half0, const float* half1, const float* feat_coarse,
                   const float* feat, int width, int rows, float* out0, float* out1, const char** why) {
  const rt_upsample_opts opt = o ? *o : up_default_opts();
  if ((*why = up_args_error(opt, half0, half1, feat_coarse, feat, width, rows, out0, out1)) != nullptr) return RT_E_ARG;
  const int s = opt.scale, cw = up_coarse(width, s), ch = up_coarse(rows, s);
  const UpPlain src{half0, half1, feat_coarse, cw};
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < width; ++x) {
      const size_t i = static_cast<size_t>(y) * width + x;
      const float* fp = feat + RT_FEAT_CHANNELS * i;
      if (half1)
        up_pixel<true>(src, x, y, s, cw, ch, opt.normal_pow2, opt.sigma_z, fp, out0 + 3 * i, out1 + 3 * i);
      else
        up_pixel<false>(src, x, y, s, cw, ch, opt.normal_pow2, opt.sigma_z, fp, out0 + 3 * i, nullptr);
    }
  return RT_OK;
}

#if defined(__HIPCC__) && defined(RT_UPSAMPLE_KERNEL)
// -------------------------------------------------------------- the kernel ----
// A workgroup is kDnBx x kDnBy fine pixels, a wave one row of 64; thread (x, y)
// owns fine pixel (x, y).  The workgroup first stages the coarse pixels its
// taps can touch: along an axis of n fine pixels the first taps of the first
// and the last pixel lie floor((n - 1) / S) or one more apart (up_axis), and
// the last pixel's second tap is one further, so (n + S - 1) / S + 2 coarse
// pixels bound the tile: 34 x 4 at S = 2, 24 x 4 at S = 3, 18 x 3 at S = 4.
// A coarse pixel is divided by its albedo once, at staging, and kept as three
// 16-byte words (i0 rgb, i1 r | i1 gb, n xy | n z, depth, 1 - cov, 0): 6,528
// bytes at S = 2.  Words of the tile outside the coarse image are never
// written and never read (a tap outside it is skipped before its load).
template <int S>
struct UpTile {
  static constexpr int kW = (kDnBx + S - 1) / S + 2, kH = (kDnBy + S - 1) / S + 2, kN = kW * kH;
  const float4* w;   // 3 words a coarse pixel
  int X0, Y0;        // the coarse position of the tile's first pixel
  __device__ __forceinline__ UpCoarse tap(int X, int Y) const {
    const int i = 3 * ((Y - Y0) * kW + (X - X0));
    const float4 a = w[i], b = w[i + 1], c = w[i + 2];
    UpCoarse q;
    q.i0[0] = a.x, q.i0[1] = a.y, q.i0[2] = a.z;
    q.i1[0] = a.w, q.i1[1] = b.x, q.i1[2] = b.y;
    q.g = DnGuide{b.z, b.w, c.x, c.y};
    q.omc = c.z;
    return q;
  }
};

// The fine feature row is read as 8 and the outputs are written as 3
// consecutive floats a thread; they need a float's alignment only (the
// compiler merges them into dwordx4 loads and dwordx3 stores, which global
// memory takes at any dword address).
template <int S, bool TWO>
__global__ __launch_bounds__(kDnBx* kDnBy) void upsample_kernel(const float* __restrict__ half0,
                                                                const float* __restrict__ half1,
                                                                const float* __restrict__ feat_coarse,
                                                                const float* __restrict__ feat, int width, int rows,
                                                                int normal_pow2, float sigma_z,
                                                                float* __restrict__ out0, float* __restrict__ out1) {
  using T = UpTile<S>;
  __shared__ float4 s_w[3 * T::kN];
  const int cw = up_coarse(width, S), ch = up_coarse(rows, S);
  const int fx0 = static_cast<int>(blockIdx.x) * kDnBx, fy0 = static_cast<int>(blockIdx.y) * kDnBy;
  int X0, Y0;
  float unused0, unused1;
  up_axis(fx0, S, &X0, &unused0, &unused1);
  up_axis(fy0, S, &Y0, &unused0, &unused1);
  for (int i = static_cast<int>(threadIdx.y) * kDnBx + static_cast<int>(threadIdx.x); i < T::kN; i += kDnBx * kDnBy) {
    const int ly = i / T::kW, X = X0 + (i - ly * T::kW), Y = Y0 + ly;
    if (X >= 0 && X < cw && Y >= 0 && Y < ch) {
      const size_t j = static_cast<size_t>(Y) * cw + X;
      float h0[3], h1[3] = {0.0f, 0.0f, 0.0f}, f[RT_FEAT_CHANNELS];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        h0[c] = half0[j * 3 + c];
        if (TWO) h1[c] = half1[j * 3 + c];
      }
#pragma unroll
      for (int c = 0; c < RT_FEAT_CHANNELS; ++c) f[c] = feat_coarse[j * RT_FEAT_CHANNELS + c];
      const UpCoarse q = up_coarse_pixel(h0, TWO ? h1 : nullptr, f);
      s_w[3 * i] = make_float4(q.i0[0], q.i0[1], q.i0[2], q.i1[0]);
      s_w[3 * i + 1] = make_float4(q.i1[1], q.i1[2], q.g.nx, q.g.ny);
      s_w[3 * i + 2] = make_float4(q.g.nz, q.g.z, q.omc, 0.0f);
    }
  }
  __syncthreads();
  const int x = fx0 + static_cast<int>(threadIdx.x), y = fy0 + static_cast<int>(threadIdx.y);
  if (x >= width || y >= rows) return;
  const size_t i = static_cast<size_t>(y) * width + x;
  float fp[RT_FEAT_CHANNELS], o0[3], o1[3];
#pragma unroll
  for (int c = 0; c < RT_FEAT_CHANNELS; ++c) fp[c] = feat[i * RT_FEAT_CHANNELS + c];
  const T tile{s_w, X0, Y0};
  up_pixel<TWO>(tile, x, y, S, cw, ch, normal_pow2, sigma_z, fp, o0, o1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out0[i * 3 + c] = o0[c];
    if (TWO) out1[i * 3 + c] = o1[c];
  }
}
#endif  // __HIPCC__ && RT_UPSAMPLE_KERNEL

}  // namespace rtclj
