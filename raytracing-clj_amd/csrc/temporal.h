// temporal.h — temporal accumulation (rt_temporal_*, include/rt.h): the
// accumulated half-frames of the frames already drawn, reprojected through
// rt_feat_resolve's first-hit depth into the current camera and blended with
// the current halves -- the temporal half of SVGF (Schied et al. 2017), whose
// spatial half is denoise.h.  The two halves are accumulated separately, so
// they stay independent estimates and rt_denoise's variance term shrinks on
// its own as the history builds.
//
// Replaces nothing the reference computes: it consumes what compute-pixel's
// loop (src/raytracing.clj:141-155) leaves in rt_accum / rt_adapt / rt_feat,
// one frame after another.
//
// Three parts, as denoise.h.
//  1. The definition as plain inline functions that compile for the device
//     (the kernel below) and for the host (rt_temporal_host): one pixel of one
//     step.  One text for both: every line is one fp32 operation rounded once,
//     in rt.h's order (built with -ffp-contract=off); / and sqrt are IEEE on
//     either side.  A pixel reads the history through a `Src` -- three
//     accessors -- so the host may keep it as plain arrays and the device as
//     16-byte words.
//  2. The step on the host, checks included (tp_host_step): what
//     rt_temporal_host runs, and what tools/temporal_check.cpp runs under the
//     sanitizers.
//  3. The device kernel (under __HIPCC__ and RT_TEMPORAL_KERNEL): one thread
//     per pixel, no atomics, no scratch; the bits cannot depend on the launch
//     shape.
// Moving bodies (rt_temporal_step_motion): tp_pixel<MOTION>
// takes the displacement of the pixel's body as a parameter (tp_motion: the
// row of a per-body table, by the pixel's id from body_ids.h) and subtracts it
// in step 2; the MOTION = false instantiation never reads it and is the text
// above unchanged.  tp_host_step_any and a second kernel carry both.
// The colour clamp (rt_temporal_step_clamp): tp_clamp_box is
// one pixel's box from the current frame, read through a `Cur` -- two accessors
// -- so that the host's arrays and the box kernel's LDS tile share one text;
// tp_pixel<MOTION, CLAMP> takes the box as a parameter and clamps the fetched
// history to it in step 6; the CLAMP = false instantiations never read it and
// are the texts above unchanged.  The box kernel and a clamped step kernel
// close the file.
// The budget (rt_temporal_probe, rt_temporal_step_budget):
// tp_pixel<.., WEIGHT> takes the frame's weight wt (tp_weight of the tile's
// sample multiplier) into step 6, and tp_pixel<.., PROBE> is steps 1-5 alone --
// no colour is read or written, the returned float is the history length the
// step would accept.  The WEIGHT = PROBE = false instantiations are the texts
// above unchanged.  tp_host_probe, the probe kernel and the weighted step
// kernel carry them.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "denoise.h"

namespace rtclj {

// A history word: (a0 rgb, L) or (a1 rgb, 0).
struct alignas(16) TpWord {
  float r, g, b, l;
};

constexpr int kTpMaxHistory = 65536;

// rt.h's defaults
RT_DN_FN rt_temporal_opts tp_default_opts() {
  rt_temporal_opts o;
  o.max_history = 32;
  o.sigma_z = 0.1f;
  o.normal_min = 0.9f;
  return o;
}
// nullptr, or which rule of rt.h's table the options break
inline const char* tp_opts_error(const rt_temporal_opts& o) {
  if (o.max_history < 1 || o.max_history > kTpMaxHistory) return "max_history outside 1..65536";
  if (!(o.sigma_z > 0.0f) || !(o.sigma_z < INFINITY)) return "sigma_z is not finite and > 0";
  if (!(o.normal_min >= -1.0f) || !(o.normal_min <= 1.0f)) return "normal_min outside -1..1";
  return nullptr;
}
// rt.h's defaults of the clamp
constexpr int kTpMaxRadius = 3;
RT_DN_FN rt_temporal_clamp_opts tp_default_clamp_opts() {
  rt_temporal_clamp_opts k;
  k.radius = 2;
  k.gamma = 1.0f;
  return k;
}
inline const char* tp_clamp_opts_error(const rt_temporal_clamp_opts& k) {
  if (k.radius < 1 || k.radius > kTpMaxRadius) return "radius outside 1..3";
  if (!(k.gamma > 0.0f)) return "gamma is not > 0";
  return nullptr;
}
// nullptr, or what is wrong with an image of rows x width whose first row is
// camera row row0 (the kernel's grid has a block row per kDnBy image rows)
inline const char* tp_shape_error(int width, int rows, int row0) {
  if (width <= 0 || rows <= 0 || static_cast<int64_t>(width) * rows > 0x7fffffffll) return "bad width/rows";
  if (row0 < 0 || static_cast<int64_t>(row0) + rows > 0x7fffffffll) return "bad row0";
  return nullptr;
}

// What one step needs besides the arrays: the current camera's pinhole part,
// the previous camera's inverse basis R (rows R0, R1, R2) and dc = center -
// center', the image and the options.  The kernel takes it by value.
struct TpFrame {
  float center[3], p00[3], du[3], dv[3];
  float R[9], dc[3];
  int width, rows, row0, have_prev;
  float max_history, sigma_z, normal_min;
};

// The host set-up of a step (rt.h): R and dc from the previous camera, in
// double on its fp32 fields.  false: det is 0 or not finite.
inline bool tp_setup(const rt_camera& cur, const rt_camera& prev, float* R9, float* dc3) {
  double q[3], du[3], dv[3];
  for (int c = 0; c < 3; ++c) {
    q[c] = static_cast<double>(prev.p00[c]) - static_cast<double>(prev.center[c]);
    du[c] = prev.du[c];
    dv[c] = prev.dv[c];
  }
  auto cross = [](const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
  };
  double c0[3], c1[3], c2[3];
  cross(dv, q, c0);
  cross(q, du, c1);
  cross(du, dv, c2);
  const double det = (du[0] * c0[0] + du[1] * c0[1]) + du[2] * c0[2];
  if (det == 0.0 || !std::isfinite(det)) return false;
  for (int c = 0; c < 3; ++c) {
    R9[c] = static_cast<float>(c0[c] / det);
    R9[3 + c] = static_cast<float>(c1[c] / det);
    R9[6 + c] = static_cast<float>(c2[c] / det);
    dc3[c] = cur.center[c] - prev.center[c];
  }
  return true;
}

inline TpFrame tp_frame(const rt_temporal_opts& o, const rt_camera& cam, int width, int rows, int row0) {
  TpFrame f{};
  for (int c = 0; c < 3; ++c) {
    f.center[c] = cam.center[c];
    f.p00[c] = cam.p00[c];
    f.du[c] = cam.du[c];
    f.dv[c] = cam.dv[c];
  }
  f.width = width;
  f.rows = rows;
  f.row0 = row0;
  f.have_prev = 0;
  f.max_history = static_cast<float>(o.max_history);
  f.sigma_z = o.sigma_z;
  f.normal_min = o.normal_min;
  return f;
}

RT_DN_FN float tp_floor(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return floorf(x);
#else
  return std::floor(x);
#endif
}
RT_DN_FN bool tp_finite(float x) { return dn_abs(x) < INFINITY; }

// One axis of step 4: the tap's first index and its fraction, snapped.  f is
// inside (-1, size) here, so the conversion is in range.
RT_DN_FN void tp_split(float f, int* i0, float* t) {
  const float fl = tp_floor(f);
  int i = static_cast<int>(fl);
  float tt = f - fl;
  if (tt < 0x1p-6f) {
    tt = 0.0f;
  } else if (tt > 1.0f - 0x1p-6f) {
    i += 1;
    tt = 0.0f;
  }
  *i0 = i;
  *t = tt;
}

// The colour box of pixel (x, y) of a rows x width band (rt.h, the clamp):
// lo, hi (3 floats each) from the current frame's halves and guides over the
// (2 radius + 1)^2 window.  Cur:
//   DnGuide guide(int x, int y)                         feat[3..6]
//   void halves(int x, int y, float* h0, float* h1)     3 floats each
// called for pixels inside the band only; a tap's guide is read before, and
// its halves only after, it has passed the surface tests.
template <class Cur>
RT_DN_FN void tp_clamp_box(const Cur& cur, int x, int y, int width, int rows, int radius, float sigma_z,
                           float normal_min, float gamma, float* lo, float* hi) {
  const DnGuide gp = cur.guide(x, y);
  const bool pinf = gp.z == INFINITY, pfin = tp_finite(gp.z);
  const float tol = sigma_z * gp.z;
  float s1[3] = {0.0f, 0.0f, 0.0f}, s2[3] = {0.0f, 0.0f, 0.0f}, cnt = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -radius; dy <= radius; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -radius; dx <= radius; ++dx) {
      // (|d| <= 3: no overflow for any int x, y inside the band)
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
      if (dx != 0 || dy != 0) {   // (the centre is always valid)
        const DnGuide g = cur.guide(qx, qy);
        if (!(pinf && g.z == INFINITY)) {
          if (!(pfin && tp_finite(g.z))) continue;
          if (!(dn_abs(g.z - gp.z) <= tol)) continue;
          const float dot = (gp.nx * g.nx + gp.ny * g.ny) + gp.nz * g.nz;
          if (!(dot >= normal_min)) continue;
        }
      }
      float h0[3], h1[3];
      cur.halves(qx, qy, h0, h1);
      for (int c = 0; c < 3; ++c) {
        s1[c] += h0[c];
        s2[c] += h0[c] * h0[c];
      }
      cnt += 1.0f;
      for (int c = 0; c < 3; ++c) {
        s1[c] += h1[c];
        s2[c] += h1[c] * h1[c];
      }
      cnt += 1.0f;
    }
  }
  for (int c = 0; c < 3; ++c) {
    const float mean = s1[c] / cnt;
    float var = s2[c] / cnt - mean * mean;
    var = var > 0.0f ? var : 0.0f;
    const float e = gamma * dn_sqrt(var);
    lo[c] = mean - e;
    hi[c] = mean + e;
  }
}

// One pixel (x, y) of a step: o0, o1 (3 floats each) and the returned length
// N from the current halves h0, h1 (3 floats each), the current features feat
// (8 floats) and the history.  Src:
//   TpWord w0(size_t i)   (a0 rgb, L) of history pixel i = y * width + x
//   TpWord w1(size_t i)   (a1 rgb, -)
//   DnGuide guide(size_t i)
// read for pixels inside the image only, and only with f.have_prev.
// MOTION (rt_temporal_step_motion): m (3 floats) is the displacement of the
// pixel's body since the previous frame (tp_motion), subtracted in step 2;
// without it m is not read and the text is rt_temporal_step's.
// CLAMP (rt_temporal_step_clamp): box (6 floats: lo rgb, hi rgb; tp_clamp_box)
// bounds the fetched history in step 6; without it box is not read.
// WEIGHT (rt_temporal_step_budget): the current halves stand for wt frames'
// worth of samples (tp_weight), so step 6 adds wt to the length and blends with
// k = wt / N; without it wt is not read.
// PROBE (rt_temporal_probe): steps 1-5 only -- h0, h1, o0, o1 and box are not
// touched; of the history only Src's hist_len(i) and the guides of the taps
// with L >= 1 are read -- and the return is Lh = accL / bsum where the step
// would accept the history, else 0.
template <bool MOTION, bool CLAMP = false, bool WEIGHT = false, bool PROBE = false, class Src>
RT_DN_FN float tp_pixel(const Src& src, const TpFrame& f, int x, int y, const float* h0, const float* h1,
                        const float* feat, const float* m, float* o0, float* o1, const float* box = nullptr,
                        float wt = 1.0f) {
  bool hist = f.have_prev != 0;
  float fx = 0.0f, fy = 0.0f, zexp = INFINITY;
  if (hist) {
    // 1. the pixel centre's pinhole ray
    const float xf = static_cast<float>(x), jf = static_cast<float>(f.row0 + y);
    float e[3], w[3];
    for (int c = 0; c < 3; ++c) e[c] = ((f.p00[c] + xf * f.du[c]) + jf * f.dv[c]) - f.center[c];
    // 2. the surface point relative to the previous camera's centre
    const float zp = feat[6];
    if (tp_finite(zp)) {
      const float len = dn_sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
      const float sc = zp / len;
      for (int c = 0; c < 3; ++c) w[c] = MOTION ? (sc * e[c] + f.dc[c]) - m[c] : sc * e[c] + f.dc[c];
      zexp = dn_sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    } else {
      for (int c = 0; c < 3; ++c) w[c] = e[c];
    }
    // 3. where the previous camera saw it (NaN fails every comparison)
    const float al = (f.R[0] * w[0] + f.R[1] * w[1]) + f.R[2] * w[2];
    const float be = (f.R[3] * w[0] + f.R[4] * w[1]) + f.R[5] * w[2];
    const float ga = (f.R[6] * w[0] + f.R[7] * w[1]) + f.R[8] * w[2];
    hist = ga > 0.0f;
    if (hist) {
      fx = al / ga;
      fy = be / ga - static_cast<float>(f.row0);
      hist = fx > -1.0f && fx < static_cast<float>(f.width) && fy > -1.0f && fy < static_cast<float>(f.rows);
    }
  }
  float acc0[3] = {0.0f, 0.0f, 0.0f}, acc1[3] = {0.0f, 0.0f, 0.0f}, accl = 0.0f, bsum = 0.0f;
  if (hist) {
    // 4. the 2 x 2 taps' corner and fractions
    int x0, y0;
    float tx, ty;
    tp_split(fx, &x0, &tx);
    tp_split(fy, &y0, &ty);
    const float tol = f.sigma_z * zexp;
    const bool pinf = zexp == INFINITY, pfin = tp_finite(zexp);
    // 5. the valid taps
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dy = 0; dy <= 1; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int dx = 0; dx <= 1; ++dx) {
        const float b = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
        const int qx = x0 + dx, qy = y0 + dy;
        if (b == 0.0f || qx < 0 || qx >= f.width || qy < 0 || qy >= f.rows) continue;
        const size_t q = static_cast<size_t>(qy) * f.width + qx;
        TpWord a{0.0f, 0.0f, 0.0f, 0.0f};
        if (PROBE) a.l = src.hist_len(q);
        else a = src.w0(q);
        if (!(a.l >= 1.0f)) continue;
        const DnGuide g = src.guide(q);
        if (!(pinf && g.z == INFINITY)) {
          if (!(pfin && tp_finite(g.z))) continue;
          if (!(dn_abs(g.z - zexp) <= tol)) continue;
          const float dot = (feat[3] * g.nx + feat[4] * g.ny) + feat[5] * g.nz;
          if (!(dot >= f.normal_min)) continue;
        }
        if (!PROBE) {
          const TpWord a1 = src.w1(q);
          acc0[0] += b * a.r;
          acc0[1] += b * a.g;
          acc0[2] += b * a.b;
          acc1[0] += b * a1.r;
          acc1[1] += b * a1.g;
          acc1[2] += b * a1.b;
        }
        accl += b * a.l;
        bsum += b;
      }
    }
  }
  if (PROBE) return (hist && bsum >= 0.25f) ? accl / bsum : 0.0f;
  // 6. the blend
  if (hist && bsum >= 0.25f) {
    const float lh = accl / bsum;
    const float n = dn_min(WEIGHT ? lh + wt : lh + 1.0f, f.max_history);
    const float k = WEIGHT ? wt / n : 1.0f / n;
    for (int c = 0; c < 3; ++c) {
      float a = acc0[c] / bsum, b = acc1[c] / bsum;
      if (CLAMP) {   // (NaN bounds -- gamma = +inf over a constant window -- fail both comparisons)
        const float lo = box[c], hi = box[3 + c];
        a = a < lo ? lo : (a > hi ? hi : a);
        b = b < lo ? lo : (b > hi ? hi : b);
      }
      o0[c] = a + k * (h0[c] - a);
      o1[c] = b + k * (h1[c] - b);
    }
    return n;
  }
  for (int c = 0; c < 3; ++c) {
    o0[c] = h0[c];
    o1[c] = h1[c];
  }
  return WEIGHT ? dn_min(wt, f.max_history) : 1.0f;
}

// The weight of a frame whose tile was traced at `mult` times the base rate
// (rt.h, the weighted step): float(min(max(mult, 1), 16)).
constexpr uint32_t kTpMaxWeight = 16u;
RT_DN_FN float tp_weight(uint32_t mult) {
  return static_cast<float>(mult < 1u ? 1u : (mult > kTpMaxWeight ? kTpMaxWeight : mult));
}
// ... of pixel (x, y) of the band: its 8 x 8 tile's entry of the gy x gx table
constexpr int kTpTile = 8;
RT_DN_FN float tp_weight_at(const uint32_t* mult, int width, int x, int y) {
  const int gx = (width + kTpTile - 1) / kTpTile;
  return tp_weight(mult[static_cast<size_t>(y / kTpTile) * gx + x / kTpTile]);
}

// The current frame as plain arrays (the host): half0, half1 rows x width x 3,
// feat rows x width x 8.
struct TpCurPlain {
  const float *h0, *h1, *feat;
  int width;
  size_t at(int x, int y) const { return static_cast<size_t>(y) * width + x; }
  DnGuide guide(int x, int y) const {
    const float* ft = feat + RT_FEAT_CHANNELS * at(x, y);
    return DnGuide{ft[3], ft[4], ft[5], ft[6]};
  }
  void halves(int x, int y, float* a, float* b) const {
    const size_t i = 3 * at(x, y);
    for (int c = 0; c < 3; ++c) {
      a[c] = h0[i + c];
      b[c] = h1[i + c];
    }
  }
};

// The history as plain arrays (the host): a0, a1 rows x width x 3, guide
// rows x width x 4, len rows x width.
struct TpPlain {
  const float *a0, *a1, *g, *len;
  TpWord w0(size_t i) const { return TpWord{a0[3 * i], a0[3 * i + 1], a0[3 * i + 2], len[i]}; }
  TpWord w1(size_t i) const { return TpWord{a1[3 * i], a1[3 * i + 1], a1[3 * i + 2], 0.0f}; }
  float hist_len(size_t i) const { return len[i]; }   // (the probe: a0 and a1 may be nullptr)
  DnGuide guide(size_t i) const { return DnGuide{g[4 * i], g[4 * i + 1], g[4 * i + 2], g[4 * i + 3]}; }
};

inline bool tp_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

// Step 2's displacement of a pixel whose body is b = ids[p] (rt.h): row b of
// `motion` (n_bodies x 4 floats) if 0 <= b < n_bodies, else (0, 0, 0).  The
// range test is on the integer, before any load of the table.
RT_DN_FN void tp_motion(int32_t b, const float* motion, int n_bodies, float* m) {
  m[0] = m[1] = m[2] = 0.0f;
  if (static_cast<uint32_t>(b) < static_cast<uint32_t>(n_bodies)) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 row = reinterpret_cast<const float4*>(motion)[b];   // one 16-byte load (the table is 16-byte aligned)
    m[0] = row.x, m[1] = row.y, m[2] = row.z;
#else
    for (int c = 0; c < 3; ++c) m[c] = motion[4 * static_cast<size_t>(b) + c];
#endif
  }
}
// what the motion-aware step asks of its extra arguments, or nullptr
inline const char* tp_motion_error(const int32_t* ids, const float* motion, int n_bodies) {
  if (!ids) return "NULL argument";
  if (n_bodies < 0) return "n_bodies < 0";
  if (n_bodies > 0 && !motion) return "NULL argument";
  return nullptr;
}

// rt_temporal_host, rt_temporal_host_motion and rt_temporal_host_clamp (rt.h):
// the checks, then every pixel.  0, or RT_E_ARG with *why set.  k is looked at
// with CLAMP only (nullptr: the defaults).  WEIGHT (rt_temporal_host_budget):
// mult is the band's gy x gx table of sample multipliers; without it mult is
// not looked at.
template <bool MOTION, bool CLAMP = false, bool WEIGHT = false>
inline int tp_host_step_any(const rt_temporal_opts* o, const rt_temporal_clamp_opts* k, const rt_camera* cam,
                            const rt_camera* prev_cam, int width,
                            int rows, int row0, const float* half0, const float* half1, const float* feat,
                            const float* prev_a0, const float* prev_a1, const float* prev_guide, const float* prev_len,
                            const int32_t* ids, const float* motion, int n_bodies, float* out0, float* out1,
                            float* out_len, const char** why, const uint32_t* mult = nullptr) {
  *why = nullptr;
  if (!cam || !half0 || !half1 || !feat || !out0 || !out1 || !out_len || (WEIGHT && !mult) ||
      (prev_cam && (!prev_a0 || !prev_a1 || !prev_guide || !prev_len))) {
    *why = "NULL argument";
    return RT_E_ARG;
  }
  if (MOTION && (*why = tp_motion_error(ids, motion, n_bodies)) != nullptr) return RT_E_ARG;
  if ((*why = tp_shape_error(width, rows, row0)) != nullptr) return RT_E_ARG;
  const rt_temporal_opts opt = o ? *o : tp_default_opts();
  if ((*why = tp_opts_error(opt)) != nullptr) return RT_E_ARG;
  const rt_temporal_clamp_opts kopt = CLAMP && k ? *k : tp_default_clamp_opts();
  if (CLAMP && (*why = tp_clamp_opts_error(kopt)) != nullptr) return RT_E_ARG;
  const size_t n_px = static_cast<size_t>(width) * rows, fb = sizeof(float);
  const void* outs[3] = {out0, out1, out_len};
  const size_t out_b[3] = {n_px * 3 * fb, n_px * 3 * fb, n_px * fb};
  const size_t n_tiles = static_cast<size_t>((width + kTpTile - 1) / kTpTile) * ((rows + kTpTile - 1) / kTpTile);
  const void* ins[10] = {half0,      half1,    feat, prev_a0, prev_a1,
                         prev_guide, prev_len, MOTION ? ids : nullptr, MOTION ? motion : nullptr,
                         WEIGHT ? mult : nullptr};
  const size_t in_b[10] = {n_px * 3 * fb, n_px * 3 * fb, n_px * RT_FEAT_CHANNELS * fb,
                           n_px * 3 * fb, n_px * 3 * fb, n_px * 4 * fb,
                           n_px * fb,     n_px * sizeof(int32_t), static_cast<size_t>(MOTION ? n_bodies : 0) * 4 * fb,
                           n_tiles * sizeof(uint32_t)};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 10; ++b)
      if ((b < 3 || b > 6 || prev_cam) && tp_overlap(outs[a], out_b[a], ins[b], in_b[b])) {
        *why = "an output overlaps an input";
        return RT_E_ARG;
      }
    for (int b = a + 1; b < 3; ++b)
      if (tp_overlap(outs[a], out_b[a], outs[b], out_b[b])) {
        *why = "the outputs overlap";
        return RT_E_ARG;
      }
  }
  TpFrame f = tp_frame(opt, *cam, width, rows, row0);
  if (prev_cam) {
    if (!tp_setup(*cam, *prev_cam, f.R, f.dc)) {
      *why = "the previous camera is degenerate (det is 0 or not finite)";
      return RT_E_ARG;
    }
    f.have_prev = 1;
  }
  const TpPlain src{prev_a0, prev_a1, prev_guide, prev_len};
  const TpCurPlain cur{half0, half1, feat, width};
  (void)cur;
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < width; ++x) {
      const size_t i = static_cast<size_t>(y) * width + x;
      const float* ft = feat + RT_FEAT_CHANNELS * i;
      float m[3] = {0.0f, 0.0f, 0.0f}, box[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (MOTION && tp_finite(ft[6])) tp_motion(ids[i], motion, n_bodies, m);   // (a sky pixel ignores its id)
      if (CLAMP && f.have_prev)   // (without a previous camera no pixel has history to clamp)
        tp_clamp_box(cur, x, y, width, rows, kopt.radius, f.sigma_z, f.normal_min, kopt.gamma, box, box + 3);
      out_len[i] = tp_pixel<MOTION, CLAMP, WEIGHT>(src, f, x, y, half0 + 3 * i, half1 + 3 * i, ft, m, out0 + 3 * i,
                                                   out1 + 3 * i, box, WEIGHT ? tp_weight_at(mult, width, x, y) : 1.0f);
    }
  return RT_OK;
}
inline int tp_host_step(const rt_temporal_opts* o, const rt_camera* cam, const rt_camera* prev_cam, int width,
                        int rows, int row0, const float* half0, const float* half1, const float* feat,
                        const float* prev_a0, const float* prev_a1, const float* prev_guide, const float* prev_len,
                        float* out0, float* out1, float* out_len, const char** why) {
  return tp_host_step_any<false>(o, nullptr, cam, prev_cam, width, rows, row0, half0, half1, feat, prev_a0, prev_a1,
                                 prev_guide, prev_len, nullptr, nullptr, 0, out0, out1, out_len, why);
}
inline int tp_host_step_motion(const rt_temporal_opts* o, const rt_camera* cam, const rt_camera* prev_cam, int width,
                               int rows, int row0, const float* half0, const float* half1, const float* feat,
                               const float* prev_a0, const float* prev_a1, const float* prev_guide,
                               const float* prev_len, const int32_t* ids, const float* motion, int n_bodies,
                               float* out0, float* out1, float* out_len, const char** why) {
  return tp_host_step_any<true>(o, nullptr, cam, prev_cam, width, rows, row0, half0, half1, feat, prev_a0, prev_a1,
                                prev_guide, prev_len, ids, motion, n_bodies, out0, out1, out_len, why);
}
// ids == nullptr: rt_temporal_host's reprojection (motion and n_bodies are not read)
inline int tp_host_step_clamp(const rt_temporal_opts* o, const rt_temporal_clamp_opts* k, const rt_camera* cam,
                              const rt_camera* prev_cam, int width, int rows, int row0, const float* half0,
                              const float* half1, const float* feat, const float* prev_a0, const float* prev_a1,
                              const float* prev_guide, const float* prev_len, const int32_t* ids, const float* motion,
                              int n_bodies, float* out0, float* out1, float* out_len, const char** why) {
  if (!ids)
    return tp_host_step_any<false, true>(o, k, cam, prev_cam, width, rows, row0, half0, half1, feat, prev_a0, prev_a1,
                                         prev_guide, prev_len, nullptr, nullptr, 0, out0, out1, out_len, why);
  return tp_host_step_any<true, true>(o, k, cam, prev_cam, width, rows, row0, half0, half1, feat, prev_a0, prev_a1,
                                      prev_guide, prev_len, ids, motion, n_bodies, out0, out1, out_len, why);
}
// rt_temporal_host_budget (rt.h): rt_temporal_host_clamp's step with the tiles'
// weights in step 6.  gamma = +inf clamps nothing (rt.h), so the box is not
// built then.
inline int tp_host_step_budget(const rt_temporal_opts* o, const rt_temporal_clamp_opts* k, const rt_camera* cam,
                               const rt_camera* prev_cam, int width, int rows, int row0, const float* half0,
                               const float* half1, const float* feat, const float* prev_a0, const float* prev_a1,
                               const float* prev_guide, const float* prev_len, const int32_t* ids, const float* motion,
                               int n_bodies, const uint32_t* mult, float* out0, float* out1, float* out_len,
                               const char** why) {
  if (k && (*why = tp_clamp_opts_error(*k)) != nullptr) return RT_E_ARG;
  const bool box = !(k && k->gamma == INFINITY);
#define RT_TP_BUDGET(MOTION, CLAMP, IDS, MOT, NB)                                                                     \
  tp_host_step_any<MOTION, CLAMP, true>(o, k, cam, prev_cam, width, rows, row0, half0, half1, feat, prev_a0, prev_a1, \
                                        prev_guide, prev_len, IDS, MOT, NB, out0, out1, out_len, why, mult)
  if (!ids) return box ? RT_TP_BUDGET(false, true, nullptr, nullptr, 0) : RT_TP_BUDGET(false, false, nullptr, nullptr, 0);
  return box ? RT_TP_BUDGET(true, true, ids, motion, n_bodies) : RT_TP_BUDGET(true, false, ids, motion, n_bodies);
#undef RT_TP_BUDGET
}

// rt_temporal_host_probe (rt.h): the checks, then steps 1-5 of every pixel.
// ids == nullptr: the plain step 2 (motion and n_bodies are not read).
template <bool MOTION>
inline int tp_host_probe_any(const rt_temporal_opts* o, const rt_camera* cam, const rt_camera* prev_cam, int width,
                             int rows, int row0, const float* feat, const float* prev_guide, const float* prev_len,
                             const int32_t* ids, const float* motion, int n_bodies, float* out_len, const char** why) {
  *why = nullptr;
  if (!cam || !feat || !out_len || (prev_cam && (!prev_guide || !prev_len))) {
    *why = "NULL argument";
    return RT_E_ARG;
  }
  if (MOTION && (*why = tp_motion_error(ids, motion, n_bodies)) != nullptr) return RT_E_ARG;
  if ((*why = tp_shape_error(width, rows, row0)) != nullptr) return RT_E_ARG;
  const rt_temporal_opts opt = o ? *o : tp_default_opts();
  if ((*why = tp_opts_error(opt)) != nullptr) return RT_E_ARG;
  const size_t n_px = static_cast<size_t>(width) * rows, fb = sizeof(float);
  const void* ins[5] = {feat, prev_cam ? prev_guide : nullptr, prev_cam ? prev_len : nullptr, MOTION ? ids : nullptr,
                        MOTION ? motion : nullptr};
  const size_t in_b[5] = {n_px * RT_FEAT_CHANNELS * fb, n_px * 4 * fb, n_px * fb, n_px * sizeof(int32_t),
                          static_cast<size_t>(MOTION ? n_bodies : 0) * 4 * fb};
  for (int b = 0; b < 5; ++b)
    if (tp_overlap(out_len, n_px * fb, ins[b], in_b[b])) {
      *why = "the output overlaps an input";
      return RT_E_ARG;
    }
  TpFrame f = tp_frame(opt, *cam, width, rows, row0);
  if (prev_cam) {
    if (!tp_setup(*cam, *prev_cam, f.R, f.dc)) {
      *why = "the previous camera is degenerate (det is 0 or not finite)";
      return RT_E_ARG;
    }
    f.have_prev = 1;
  }
  const TpPlain src{nullptr, nullptr, prev_guide, prev_len};
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < width; ++x) {
      const size_t i = static_cast<size_t>(y) * width + x;
      const float* ft = feat + RT_FEAT_CHANNELS * i;
      float m[3] = {0.0f, 0.0f, 0.0f};
      if (MOTION && tp_finite(ft[6])) tp_motion(ids[i], motion, n_bodies, m);
      out_len[i] = tp_pixel<MOTION, false, false, true>(src, f, x, y, nullptr, nullptr, ft, m, nullptr, nullptr);
    }
  return RT_OK;
}
inline int tp_host_probe(const rt_temporal_opts* o, const rt_camera* cam, const rt_camera* prev_cam, int width,
                         int rows, int row0, const float* feat, const float* prev_guide, const float* prev_len,
                         const int32_t* ids, const float* motion, int n_bodies, float* out_len, const char** why) {
  if (!ids)
    return tp_host_probe_any<false>(o, cam, prev_cam, width, rows, row0, feat, prev_guide, prev_len, nullptr, nullptr, 0,
                                    out_len, why);
  return tp_host_probe_any<true>(o, cam, prev_cam, width, rows, row0, feat, prev_guide, prev_len, ids, motion, n_bodies,
                                 out_len, why);
}

#if defined(__HIPCC__) && defined(RT_TEMPORAL_KERNEL)
// -------------------------------------------------------------- the kernel ----
// The history as the device keeps it: three 16-byte words a pixel.
struct TpPacked {
  const TpWord* a0;
  const TpWord* a1;
  const DnGuide* g;
  __device__ __forceinline__ TpWord w0(size_t i) const { return a0[i]; }
  __device__ __forceinline__ TpWord w1(size_t i) const { return a1[i]; }
  __device__ __forceinline__ float hist_len(size_t i) const { return a0[i].l; }   // (one dword of the word)
  __device__ __forceinline__ DnGuide guide(size_t i) const { return g[i]; }
};

// A workgroup is kDnBx x kDnBy pixels, a wave one row of 64; thread (x, y)
// owns pixel (x, y).  The current inputs are read as single floats (they need
// no more than a float's alignment); the history is gathered as 16-byte words
// straight from global memory -- where a tap lies depends on the data, so no
// LDS tile; the taps of neighbouring pixels are neighbours under any smooth
// motion and meet in the vector L1 and the L2 -- and the three new history
// words and both outputs are written by the owning thread.  The old and the
// new history are different buffers (rt_temporal's two sets).
// The four step kernels' thread.  MOTION adds the pixel's body id (one dword)
// and, for an id inside the table, that body's row (one 16-byte word;
// neighbouring pixels mostly share a body, and the whole table -- 16 bytes a
// body -- stays in the caches; a sky pixel loads neither); BOX the pixel's own
// two box words -- loaded only when there is a previous camera: the first step
// enqueues no box kernel; WEIGHT one dword of the tile's multiplier (a wave's
// 64 pixels lie in eight tiles of one tile row: eight dwords, one cache line).
// What a kernel's switches leave out is not read.
template <bool MOTION, bool BOX, bool WEIGHT>
__device__ __forceinline__ void tp_step_thread(
    const TpFrame& f, const float* __restrict__ half0, const float* __restrict__ half1, const float* __restrict__ feat,
    const int32_t* __restrict__ ids, const float* __restrict__ motion, const int n_bodies,
    const uint32_t* __restrict__ mult, const TpWord* __restrict__ box_lo, const TpWord* __restrict__ box_hi,
    const TpWord* __restrict__ prev_a0, const TpWord* __restrict__ prev_a1, const DnGuide* __restrict__ prev_g,
    TpWord* __restrict__ new_a0, TpWord* __restrict__ new_a1, DnGuide* __restrict__ new_g, float* __restrict__ out0,
    float* __restrict__ out1) {
  const int x = static_cast<int>(blockIdx.x) * kDnBx + static_cast<int>(threadIdx.x);
  const int y = static_cast<int>(blockIdx.y) * kDnBy + static_cast<int>(threadIdx.y);
  if (x >= f.width || y >= f.rows) return;
  const size_t i = static_cast<size_t>(y) * f.width + x;
  float h0[3], h1[3], ft[RT_FEAT_CHANNELS], o0[3], o1[3], m[3] = {0.0f, 0.0f, 0.0f};
  float box[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    h0[c] = half0[i * 3 + c];
    h1[c] = half1[i * 3 + c];
  }
#pragma unroll
  for (int c = 0; c < RT_FEAT_CHANNELS; ++c) ft[c] = feat[i * RT_FEAT_CHANNELS + c];
  if (MOTION && tp_finite(ft[6])) tp_motion(ids[i], motion, n_bodies, m);
  if (BOX && f.have_prev) {
    const TpWord lo = box_lo[i], hi = box_hi[i];
    box[0] = lo.r, box[1] = lo.g, box[2] = lo.b;
    box[3] = hi.r, box[4] = hi.g, box[5] = hi.b;
  }
  const float wt = WEIGHT ? tp_weight_at(mult, f.width, x, y) : 1.0f;
  const TpPacked src{prev_a0, prev_a1, prev_g};
  const float n = tp_pixel<MOTION, BOX, WEIGHT>(src, f, x, y, h0, h1, ft, m, o0, o1, box, wt);
  new_a0[i] = TpWord{o0[0], o0[1], o0[2], n};
  new_a1[i] = TpWord{o1[0], o1[1], o1[2], 0.0f};
  new_g[i] = DnGuide{ft[3], ft[4], ft[5], ft[6]};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out0[i * 3 + c] = o0[c];
    out1[i * 3 + c] = o1[c];
  }
}

__global__ __launch_bounds__(kDnBx* kDnBy) void temporal_step_kernel(
    const TpFrame f, const float* __restrict__ half0, const float* __restrict__ half1, const float* __restrict__ feat,
    const TpWord* __restrict__ prev_a0, const TpWord* __restrict__ prev_a1, const DnGuide* __restrict__ prev_g,
    TpWord* __restrict__ new_a0, TpWord* __restrict__ new_a1, DnGuide* __restrict__ new_g, float* __restrict__ out0,
    float* __restrict__ out1) {
  tp_step_thread<false, false, false>(f, half0, half1, feat, nullptr, nullptr, 0, nullptr, nullptr, nullptr, prev_a0,
                                      prev_a1, prev_g, new_a0, new_a1, new_g, out0, out1);
}

// rt_temporal_step_motion's kernel
__global__ __launch_bounds__(kDnBx* kDnBy) void temporal_step_motion_kernel(
    const TpFrame f, const float* __restrict__ half0, const float* __restrict__ half1, const float* __restrict__ feat,
    const int32_t* __restrict__ ids, const float* __restrict__ motion, const int n_bodies,
    const TpWord* __restrict__ prev_a0, const TpWord* __restrict__ prev_a1, const DnGuide* __restrict__ prev_g,
    TpWord* __restrict__ new_a0, TpWord* __restrict__ new_a1, DnGuide* __restrict__ new_g, float* __restrict__ out0,
    float* __restrict__ out1) {
  tp_step_thread<true, false, false>(f, half0, half1, feat, ids, motion, n_bodies, nullptr, nullptr, nullptr, prev_a0,
                                     prev_a1, prev_g, new_a0, new_a1, new_g, out0, out1);
}

// ---- the clamp (rt_temporal_step_clamp) ----
// The box kernel: a workgroup of kDnBx x kDnBy pixels first stages its pixels
// and a halo of R around them -- both halves and the four guide floats, 40
// bytes a pixel: 15,840 bytes at R = 1, 21,760 at R = 2, 28,000 at R = 3 -- in
// LDS as three arrays of 16-, 16- and 8-byte words, so that a wave's tap is 64
// consecutive words of each (ds_read_b128, ds_read_b128, ds_read_b64: every
// 16-lane group of a b128 read and every half-wave of a b64 read covers each
// bank once).  Cells of the tile that lie outside the band get a NaN depth
// and are never read (a tap outside the band is skipped before its load).
template <int R>
struct TpBoxTile {
  static constexpr int kW = kDnBx + 2 * R, kH = kDnBy + 2 * R, kN = kW * kH;
  const DnGuide* g;
  const float4* a;   // half0 rgb, half1 r
  const float2* b;   // half1 g, b
  int x0, y0;        // the band position of the tile's first cell
  __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * kW + (x - x0); }
  __device__ __forceinline__ DnGuide guide(int x, int y) const { return g[at(x, y)]; }
  __device__ __forceinline__ void halves(int x, int y, float* h0, float* h1) const {
    const int i = at(x, y);
    const float4 u = a[i];
    const float2 v = b[i];
    h0[0] = u.x, h0[1] = u.y, h0[2] = u.z;
    h1[0] = u.w, h1[1] = v.x, h1[2] = v.y;
  }
};
// Thread (x, y) owns pixel (x, y) and writes its box as two 16-byte words,
// (lo rgb, 0) into box_lo and (hi rgb, 0) into box_hi (rt_temporal's scratch).
template <int R>
__global__ __launch_bounds__(kDnBx* kDnBy) void temporal_box_kernel(
    const float* __restrict__ half0, const float* __restrict__ half1, const float* __restrict__ feat, int width,
    int rows, float sigma_z, float normal_min, float gamma, TpWord* __restrict__ box_lo, TpWord* __restrict__ box_hi) {
  using T = TpBoxTile<R>;
  __shared__ DnGuide s_g[T::kN];
  __shared__ float4 s_a[T::kN];
  __shared__ float2 s_b[T::kN];
  const int x0 = static_cast<int>(blockIdx.x) * kDnBx - R, y0 = static_cast<int>(blockIdx.y) * kDnBy - R;
  for (int i = static_cast<int>(threadIdx.y) * kDnBx + static_cast<int>(threadIdx.x); i < T::kN; i += kDnBx * kDnBy) {
    const int ly = i / T::kW, gx = x0 + (i - ly * T::kW), gy = y0 + ly;
    if (gx >= 0 && gx < width && gy >= 0 && gy < rows) {
      const size_t j = static_cast<size_t>(gy) * width + gx;
      s_g[i] = DnGuide{feat[j * RT_FEAT_CHANNELS + 3], feat[j * RT_FEAT_CHANNELS + 4], feat[j * RT_FEAT_CHANNELS + 5],
                       feat[j * RT_FEAT_CHANNELS + 6]};
      s_a[i] = make_float4(half0[j * 3], half0[j * 3 + 1], half0[j * 3 + 2], half1[j * 3]);
      s_b[i] = make_float2(half1[j * 3 + 1], half1[j * 3 + 2]);
    } else {
      s_g[i] = DnGuide{0.0f, 0.0f, 0.0f, NAN};
    }
  }
  __syncthreads();
  const int x = x0 + R + static_cast<int>(threadIdx.x), y = y0 + R + static_cast<int>(threadIdx.y);
  if (x >= width || y >= rows) return;
  const T tile{s_g, s_a, s_b, x0, y0};
  float lo[3], hi[3];
  tp_clamp_box(tile, x, y, width, rows, R, sigma_z, normal_min, gamma, lo, hi);
  const size_t i = static_cast<size_t>(y) * width + x;
  box_lo[i] = TpWord{lo[0], lo[1], lo[2], 0.0f};
  box_hi[i] = TpWord{hi[0], hi[1], hi[2], 0.0f};
}

// rt_temporal_step_clamp's step kernel (MOTION = false: ids, motion and
// n_bodies are not read)
template <bool MOTION>
__global__ __launch_bounds__(kDnBx* kDnBy) void temporal_step_clamp_kernel(
    const TpFrame f, const float* __restrict__ half0, const float* __restrict__ half1, const float* __restrict__ feat,
    const int32_t* __restrict__ ids, const float* __restrict__ motion, const int n_bodies,
    const TpWord* __restrict__ box_lo, const TpWord* __restrict__ box_hi, const TpWord* __restrict__ prev_a0,
    const TpWord* __restrict__ prev_a1, const DnGuide* __restrict__ prev_g, TpWord* __restrict__ new_a0,
    TpWord* __restrict__ new_a1, DnGuide* __restrict__ new_g, float* __restrict__ out0, float* __restrict__ out1) {
  tp_step_thread<MOTION, true, false>(f, half0, half1, feat, ids, motion, n_bodies, nullptr, box_lo, box_hi, prev_a0,
                                      prev_a1, prev_g, new_a0, new_a1, new_g, out0, out1);
}

// ---- the budget (rt_temporal_probe, rt_temporal_step_budget) ----
// rt_temporal_probe's kernel: the step kernels' thread and workgroup shape;
// a thread loads its pixel's four guide floats of the current features (the
// albedo and the coverage are not read), its body id and table row as the
// motion kernel does, and of the history the lengths of its taps (the .l dword
// of the a0 word) and, for the taps with L >= 1, their guides as 16-byte words
// -- the gather of the step without its two colour words a tap -- and stores
// one float.
template <bool MOTION>
__global__ __launch_bounds__(kDnBx* kDnBy) void temporal_probe_kernel(
    const TpFrame f, const float* __restrict__ feat, const int32_t* __restrict__ ids, const float* __restrict__ motion,
    const int n_bodies, const TpWord* __restrict__ prev_a0, const DnGuide* __restrict__ prev_g,
    float* __restrict__ out_len) {
  const int x = static_cast<int>(blockIdx.x) * kDnBx + static_cast<int>(threadIdx.x);
  const int y = static_cast<int>(blockIdx.y) * kDnBy + static_cast<int>(threadIdx.y);
  if (x >= f.width || y >= f.rows) return;
  const size_t i = static_cast<size_t>(y) * f.width + x;
  if (!f.have_prev) {   // (uniform: the first step after create or reset)
    out_len[i] = 0.0f;
    return;
  }
  float ft[RT_FEAT_CHANNELS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, m[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 3; c < 7; ++c) ft[c] = feat[i * RT_FEAT_CHANNELS + c];
  if (MOTION && tp_finite(ft[6])) tp_motion(ids[i], motion, n_bodies, m);
  const TpPacked src{prev_a0, nullptr, prev_g};
  out_len[i] = tp_pixel<MOTION, false, false, true>(src, f, x, y, nullptr, nullptr, ft, m, nullptr, nullptr);
}

// rt_temporal_step_budget's step kernel.  BOX = false (gamma = +inf, which
// clamps nothing: rt.h): no box is read.
template <bool MOTION, bool BOX>
__global__ __launch_bounds__(kDnBx* kDnBy) void temporal_step_budget_kernel(
    const TpFrame f, const float* __restrict__ half0, const float* __restrict__ half1, const float* __restrict__ feat,
    const int32_t* __restrict__ ids, const float* __restrict__ motion, const int n_bodies,
    const uint32_t* __restrict__ mult, const TpWord* __restrict__ box_lo, const TpWord* __restrict__ box_hi,
    const TpWord* __restrict__ prev_a0, const TpWord* __restrict__ prev_a1, const DnGuide* __restrict__ prev_g,
    TpWord* __restrict__ new_a0, TpWord* __restrict__ new_a1, DnGuide* __restrict__ new_g, float* __restrict__ out0,
    float* __restrict__ out1) {
  tp_step_thread<MOTION, BOX, true>(f, half0, half1, feat, ids, motion, n_bodies, mult, box_lo, box_hi, prev_a0, prev_a1,
                                    prev_g, new_a0, new_a1, new_g, out0, out1);
}
#endif  // __HIPCC__ && RT_TEMPORAL_KERNEL

}  // namespace rtclj
