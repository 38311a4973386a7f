// image.hip — what works on finished images, and knows nothing of scenes: the
// feature-guided denoiser (rt_denoiser, rt_denoise; denoise.h's kernels) and
// temporal accumulation (rt_temporal and its steps: plain, motion, clamp,
// budget, and the probe; temporal.h's kernels) and guided upsampling
// (rt_upsample; upsample.h's kernel).  DESIGN.md §3.8, §3.9, §3.10, §3.12,
// §3.13, §3.14.
#include <hip/hip_runtime.h>

#define RT_DENOISE_KERNEL
#include "denoise.h"
#define RT_TEMPORAL_KERNEL
#include "temporal.h"
#define RT_UPSAMPLE_KERNEL
#include "upsample.h"
#include "launch.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

using namespace rtclj;

// ---- the denoiser (rt.h, denoise.h) -----------------------------------------
// Its scratch on the device: the two texel arrays the levels ping-pong between
// and the guides the prep packs, for one image size.  mu orders the calls'
// enqueues (the scratch itself is ordered by the caller's stream).
struct rt_denoiser {
  int device = 0, width = 0, rows = 0;
  size_t n_px = 0;
  std::mutex mu;
  DevBuf<DnTexel> tex[2];
  DevBuf<DnGuide> guide;
  DevBuf<float> omc;
};

extern "C" int rt_denoiser_create(int device, int width, int rows, rt_denoiser** out) {
  clear_error();
  if (!out) return set_error(RT_E_ARG, "rt_denoiser_create: NULL argument");
  *out = nullptr;
  // (the level kernel's grid has a block row per kDnBy frame rows)
  if (width <= 0 || rows <= 0 || static_cast<int64_t>(width) * rows > 0x7fffffffll ||
      (rows + kDnBy - 1) / kDnBy > 65535)
    return set_error(RT_E_ARG, "rt_denoiser_create: bad width/rows");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return set_error(RT_E_NODEV, "rt_denoiser_create: device " + std::to_string(device) + " not available");
  HIP_TRY(hipSetDevice(device));
  rt_denoiser* dn = new rt_denoiser;
  dn->device = device;
  dn->width = width;
  dn->rows = rows;
  dn->n_px = static_cast<size_t>(width) * rows;
  hipError_t e = dn->tex[0].alloc(dn->n_px);
  if (e == hipSuccess) e = dn->tex[1].alloc(dn->n_px);
  if (e == hipSuccess) e = dn->guide.alloc(dn->n_px);
  if (e == hipSuccess) e = dn->omc.alloc(dn->n_px);
  if (e != hipSuccess) {
    delete dn;
    return hip_fail(e, "rt_denoiser_create");
  }
  *out = dn;
  return RT_OK;
}

extern "C" int rt_denoiser_free(rt_denoiser* dn) {
  if (!dn) return RT_OK;
  (void)hipSetDevice(dn->device);
  delete dn;
  return RT_OK;
}

static bool dn_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

// rt_denoise / rt_denoise_profile: the checks, then the prep and the levels
// enqueued on the stream.  ev (rt_denoise_profile): 2 + levels events, one
// recorded before the prep and one behind every kernel.
static int denoise_enqueue(const char* who, rt_denoiser* dn, const rt_denoise_opts* o, const float* d_half0,
                           const float* d_half1, const float* d_feat, float* d_out, void* hip_stream,
                           hipEvent_t* ev, int* levels_out) {
  const std::string me(who);
  if (!dn || !d_half0 || !d_half1 || !d_feat || !d_out) return set_error(RT_E_ARG, me + ": NULL argument");
  const rt_denoise_opts opt = o ? *o : dn_default_opts();
  if (const char* why = dn_opts_error(opt)) return set_error(RT_E_ARG, me + ": " + why);
  const size_t cb = dn->n_px * 3 * sizeof(float);
  if (dn_overlap(d_out, cb, d_half0, cb) || dn_overlap(d_out, cb, d_half1, cb) ||
      dn_overlap(d_out, cb, d_feat, dn->n_px * RT_FEAT_CHANNELS * sizeof(float)))
    return set_error(RT_E_ARG, me + ": d_out overlaps an input");
  std::lock_guard<std::mutex> lk(dn->mu);
  HIP_TRY(hipSetDevice(dn->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device(me, stream, dn->device, "the denoiser")) return rc;
  if (levels_out) *levels_out = opt.levels;
  if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
  const size_t pblocks = std::max<size_t>(1, std::min<size_t>((dn->n_px + 255) / 256, 4096));
  HIP_TRY(enqueue(denoise_prep_kernel, dim3(static_cast<unsigned>(pblocks)), dim3(256), 0, stream, d_half0, d_half1,
                  d_feat, dn->n_px, dn->tex[0].p, dn->guide.p, dn->omc.p));
  if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
  const dim3 grid(static_cast<unsigned>((dn->width + kDnBx - 1) / kDnBx),
                  static_cast<unsigned>((dn->rows + kDnBy - 1) / kDnBy)),
      block(kDnBx, kDnBy);
  for (int lv = 0; lv < opt.levels; ++lv) {
    const DnTexel* src = dn->tex[lv & 1].p;
    DnTexel* dst = dn->tex[(lv & 1) ^ 1].p;
    const bool last = lv + 1 == opt.levels;
    if (lv < 2) {   // step 1 and 2: the LDS tile
      const auto fn = lv == 0 ? (last ? denoise_level_lds_kernel<1, true> : denoise_level_lds_kernel<1, false>)
                              : (last ? denoise_level_lds_kernel<2, true> : denoise_level_lds_kernel<2, false>);
      HIP_TRY(enqueue(fn, grid, block, 0, stream, src, dn->guide.p, dn->omc.p, dn->width, dn->rows, opt.normal_pow2,
                      opt.sigma_c, opt.sigma_z, dst, d_feat, d_out));
      if (ev) HIP_TRY(hipEventRecord(ev[2 + lv], stream));
      continue;
    }
    HIP_TRY(enqueue(last ? denoise_level_kernel<true> : denoise_level_kernel<false>, grid, block, 0, stream, src,
                    dn->guide.p, dn->omc.p, dn->width, dn->rows, 1 << lv, opt.normal_pow2, opt.sigma_c, opt.sigma_z,
                    dst, d_feat, d_out));
    if (ev) HIP_TRY(hipEventRecord(ev[2 + lv], stream));
  }
  return RT_OK;
}

extern "C" int rt_denoise(rt_denoiser* dn, const rt_denoise_opts* o, const float* d_half0, const float* d_half1,
                          const float* d_feat, float* d_out, void* hip_stream) {
  clear_error();
  return denoise_enqueue("rt_denoise", dn, o, d_half0, d_half1, d_feat, d_out, hip_stream, nullptr, nullptr);
}

// rt_denoise with an event behind every kernel (diagnostic, tools/denoise_time.py):
// waits, then out_ms = {prep, level 0 .., the whole}.
extern "C" int rt_denoise_profile(rt_denoiser* dn, const rt_denoise_opts* o, const float* d_half0,
                                  const float* d_half1, const float* d_feat, float* d_out, void* hip_stream,
                                  float* out_ms) {
  clear_error();
  if (!out_ms) return set_error(RT_E_ARG, "rt_denoise_profile: NULL argument");
  if (dn) HIP_TRY(hipSetDevice(dn->device));
  hipEvent_t ev[2 + kDnMaxLevels] = {};
  hipError_t e = hipSuccess;
  for (int k = 0; dn && k < 2 + kDnMaxLevels && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
  int levels = 0;
  int rc = e == hipSuccess ? denoise_enqueue("rt_denoise_profile", dn, o, d_half0, d_half1, d_feat, d_out, hip_stream,
                                             ev, &levels)
                           : hip_fail(e, "rt_denoise_profile");
  if (rc == RT_OK) {
    e = hipEventSynchronize(ev[1 + levels]);
    for (int k = 0; k <= levels && e == hipSuccess; ++k) e = hipEventElapsedTime(&out_ms[k], ev[k], ev[k + 1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&out_ms[levels + 1], ev[0], ev[1 + levels]);
    if (e != hipSuccess) rc = hip_fail(e, "rt_denoise_profile");
  }
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  return rc;
}

// ---- temporal accumulation (rt.h, temporal.h) --------------------------------
// The history on the device: two sets of three packed arrays -- a step gathers
// from set `cur` and writes set cur ^ 1 -- and, on the host, the camera that
// wrote set `cur`.  mu orders the calls' enqueues (the sets themselves are
// ordered by the caller's stream).
struct rt_temporal {
  int device = 0, width = 0, rows = 0, row0 = 0;
  size_t n_px = 0;
  mutable std::mutex mu;
  DevBuf<TpWord> a0[2], a1[2];
  DevBuf<DnGuide> guide[2];
  DevBuf<TpWord> box;   // the clamp's scratch: n_px lo words, then n_px hi words (the first clamp step allocates it)
  int cur = 0;
  bool have_prev = false;
  rt_camera prev{};
  int64_t frames = 0;
};

extern "C" int rt_temporal_create(int device, int width, int rows, int row0, rt_temporal** out) {
  clear_error();
  if (!out) return set_error(RT_E_ARG, "rt_temporal_create: NULL argument");
  *out = nullptr;
  if (const char* why = tp_shape_error(width, rows, row0))
    return set_error(RT_E_ARG, std::string("rt_temporal_create: ") + why);
  // (the kernel's grid has a block row per kDnBy image rows)
  if ((rows + kDnBy - 1) / kDnBy > 65535) return set_error(RT_E_ARG, "rt_temporal_create: bad width/rows");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return set_error(RT_E_NODEV, "rt_temporal_create: device " + std::to_string(device) + " not available");
  HIP_TRY(hipSetDevice(device));
  rt_temporal* t = new rt_temporal;
  t->device = device;
  t->width = width;
  t->rows = rows;
  t->row0 = row0;
  t->n_px = static_cast<size_t>(width) * rows;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = t->a0[k].alloc(t->n_px);
    if (e == hipSuccess) e = t->a1[k].alloc(t->n_px);
    if (e == hipSuccess) e = t->guide[k].alloc(t->n_px);
  }
  // the set a first rt_temporal_read shows: L = 0 everywhere
  if (e == hipSuccess) e = fill_zero(t->a0[0], t->n_px, nullptr);
  if (e == hipSuccess) e = fill_zero(t->a1[0], t->n_px, nullptr);
  if (e == hipSuccess) e = fill_zero(t->guide[0], t->n_px, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    delete t;
    return hip_fail(e, "rt_temporal_create");
  }
  *out = t;
  return RT_OK;
}

extern "C" int rt_temporal_free(rt_temporal* t) {
  if (!t) return RT_OK;
  (void)hipSetDevice(t->device);
  delete t;
  return RT_OK;
}

extern "C" int rt_temporal_reset(rt_temporal* t, void* hip_stream) {
  clear_error();
  if (!t) return set_error(RT_E_ARG, "rt_temporal_reset: NULL argument");
  std::lock_guard<std::mutex> lk(t->mu);
  HIP_TRY(hipSetDevice(t->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device("rt_temporal_reset", stream, t->device, "the history")) return rc;
  HIP_TRY(fill_zero(t->a0[t->cur], t->n_px, stream));
  HIP_TRY(fill_zero(t->a1[t->cur], t->n_px, stream));
  HIP_TRY(fill_zero(t->guide[t->cur], t->n_px, stream));
  t->have_prev = false;
  t->frames = 0;
  return RT_OK;
}

extern "C" int64_t rt_temporal_frames(const rt_temporal* t) {
  if (!t) return -1;
  std::lock_guard<std::mutex> lk(t->mu);
  return t->frames;
}

// What a step and the probe share: the checks of the options (k: the clamp's,
// NULL where the call has none), of the motion table and of the outputs
// against the inputs and each other; then, under t's lock (held while *s
// lives), the frame's constants against the previous camera, the device, the
// stream and the grid.  The caller has checked its NULL arguments.
struct TpSpan {
  const void* p;
  size_t bytes;
};
struct TpSetup {
  TpFrame f;
  hipStream_t stream;
  dim3 grid, block;
  std::unique_lock<std::mutex> lock;
};
static int tp_set_up(const std::string& me, const rt_temporal* t, const rt_temporal_opts* o,
                     const rt_temporal_clamp_opts* k, const rt_camera& cam, bool motion, const int32_t* d_ids,
                     const float* d_motion, int n_bodies, const TpSpan* outs, int n_out, const TpSpan* ins, int n_in,
                     void* hip_stream, TpSetup* s) {
  if (motion) {
    if (const char* why = tp_motion_error(d_ids, d_motion, n_bodies)) return set_error(RT_E_ARG, me + ": " + why);
    if (reinterpret_cast<uintptr_t>(d_motion) % 16 != 0) return set_error(RT_E_ARG, me + ": d_motion is not 16-byte aligned");
  }
  const rt_temporal_opts opt = o ? *o : tp_default_opts();
  if (const char* why = tp_opts_error(opt)) return set_error(RT_E_ARG, me + ": " + why);
  if (k)
    if (const char* why = tp_clamp_opts_error(*k)) return set_error(RT_E_ARG, me + ": " + why);
  for (int a = 0; a < n_out; ++a)
    for (int b = 0; b < n_in; ++b)
      if (tp_overlap(outs[a].p, outs[a].bytes, ins[b].p, ins[b].bytes))
        return set_error(RT_E_ARG, me + (n_out == 1 ? ": the output" : ": an output") + " overlaps an input");
  for (int a = 1; a < n_out; ++a)
    if (tp_overlap(outs[0].p, outs[0].bytes, outs[a].p, outs[a].bytes))
      return set_error(RT_E_ARG, me + ": the outputs overlap");
  s->lock = std::unique_lock<std::mutex>(t->mu);
  s->f = tp_frame(opt, cam, t->width, t->rows, t->row0);
  if (t->have_prev) {
    if (!tp_setup(cam, t->prev, s->f.R, s->f.dc))
      return set_error(RT_E_ARG, me + ": the previous camera is degenerate (det is 0 or not finite)");
    s->f.have_prev = 1;
  }
  HIP_TRY(hipSetDevice(t->device));
  s->stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device(me, s->stream, t->device, "the history")) return rc;
  s->grid = dim3(static_cast<unsigned>((t->width + kDnBx - 1) / kDnBx), static_cast<unsigned>((t->rows + kDnBy - 1) / kDnBy));
  s->block = dim3(kDnBx, kDnBy);
  return RT_OK;
}

// rt_temporal_step (MOTION == false: d_ids, d_motion and n_bodies are not
// looked at), rt_temporal_step_motion and rt_temporal_step_clamp (CLAMP; k is
// looked at with it only): the checks, the set-up, one kernel -- with CLAMP
// and history, the box kernel before it.  WEIGHT (rt_temporal_step_budget):
// d_mult is the band's gy x gx multipliers, and CLAMP then says whether the
// box is built (k is checked either way); without it d_mult is not looked at.
template <bool MOTION, bool CLAMP, bool WEIGHT = false>
static int temporal_step(const std::string& me, rt_temporal* t, const rt_temporal_opts* o,
                         const rt_temporal_clamp_opts* k, const rt_camera* cam, const float* d_half0,
                         const float* d_half1, const float* d_feat, const int32_t* d_ids, const float* d_motion,
                         int n_bodies, float* d_out0, float* d_out1, void* hip_stream,
                         const uint32_t* d_mult = nullptr) {
  clear_error();
  if (!t || !cam || !d_half0 || !d_half1 || !d_feat || !d_out0 || !d_out1 || (WEIGHT && !d_mult))
    return set_error(RT_E_ARG, me + ": NULL argument");
  const rt_temporal_clamp_opts kopt = (CLAMP || WEIGHT) && k ? *k : tp_default_clamp_opts();
  const size_t cb = t->n_px * 3 * sizeof(float), fb = t->n_px * RT_FEAT_CHANNELS * sizeof(float);
  const size_t wb = !WEIGHT ? 0
                            : static_cast<size_t>((t->width + kTpTile - 1) / kTpTile) * ((t->rows + kTpTile - 1) / kTpTile) *
                                  sizeof(uint32_t);
  const size_t ib = MOTION ? t->n_px * sizeof(int32_t) : 0, mb = MOTION ? static_cast<size_t>(n_bodies) * 4 * sizeof(float) : 0;
  const TpSpan outs[] = {{d_out0, cb}, {d_out1, cb}};
  const TpSpan ins[] = {{d_half0, cb}, {d_half1, cb}, {d_feat, fb}, {d_ids, ib}, {d_motion, mb}, {d_mult, wb}};
  TpSetup s;
  if (const int rc = tp_set_up(me, t, o, (CLAMP || WEIGHT) ? &kopt : nullptr, *cam, MOTION, d_ids, d_motion, n_bodies, outs,
                               2, ins, 6, hip_stream, &s))
    return rc;
  const TpFrame& f = s.f;
  const hipStream_t stream = s.stream;
  const dim3 grid = s.grid, block = s.block;
  if (CLAMP && !t->box) HIP_TRY(t->box.alloc(2 * t->n_px));
  const int src = t->cur, dst = t->cur ^ 1;
  if (CLAMP) {
    TpWord *box_lo = t->box.p, *box_hi = t->box.p + t->n_px;
    const auto box_fn = kopt.radius == 1   ? temporal_box_kernel<1>
                        : kopt.radius == 2 ? temporal_box_kernel<2>
                                           : temporal_box_kernel<3>;
    if (f.have_prev)   // (the first step after create or reset has no history to clamp)
      HIP_TRY(enqueue(box_fn, grid, block, 0, stream, d_half0, d_half1, d_feat, t->width, t->rows,
                      f.sigma_z, f.normal_min, kopt.gamma, box_lo, box_hi));
    if (WEIGHT)
      HIP_TRY(enqueue(temporal_step_budget_kernel<MOTION, true>, grid, block, 0, stream, f, d_half0, d_half1, d_feat,
                      d_ids, d_motion, n_bodies, d_mult, static_cast<const TpWord*>(box_lo),
                      static_cast<const TpWord*>(box_hi), t->a0[src].p, t->a1[src].p, t->guide[src].p, t->a0[dst].p,
                      t->a1[dst].p, t->guide[dst].p, d_out0, d_out1));
    else
      HIP_TRY(enqueue(temporal_step_clamp_kernel<MOTION>, grid, block, 0, stream, f, d_half0, d_half1, d_feat, d_ids,
                      d_motion, n_bodies, static_cast<const TpWord*>(box_lo), static_cast<const TpWord*>(box_hi),
                      t->a0[src].p, t->a1[src].p, t->guide[src].p, t->a0[dst].p, t->a1[dst].p, t->guide[dst].p, d_out0,
                      d_out1));
  } else if (WEIGHT)
    HIP_TRY(enqueue(temporal_step_budget_kernel<MOTION, false>, grid, block, 0, stream, f, d_half0, d_half1, d_feat,
                    d_ids, d_motion, n_bodies, d_mult, static_cast<const TpWord*>(nullptr),
                    static_cast<const TpWord*>(nullptr), t->a0[src].p, t->a1[src].p, t->guide[src].p, t->a0[dst].p,
                    t->a1[dst].p, t->guide[dst].p, d_out0, d_out1));
  else if (MOTION)
    HIP_TRY(enqueue(temporal_step_motion_kernel, grid, block, 0, stream, f, d_half0, d_half1, d_feat, d_ids, d_motion,
                    n_bodies, t->a0[src].p, t->a1[src].p, t->guide[src].p, t->a0[dst].p, t->a1[dst].p, t->guide[dst].p,
                    d_out0, d_out1));
  else
    HIP_TRY(enqueue(temporal_step_kernel, grid, block, 0, stream, f, d_half0, d_half1, d_feat, t->a0[src].p,
                    t->a1[src].p, t->guide[src].p, t->a0[dst].p, t->a1[dst].p, t->guide[dst].p, d_out0, d_out1));
  t->cur = dst;
  t->prev = *cam;
  t->have_prev = true;
  t->frames += 1;
  return RT_OK;
}

extern "C" int rt_temporal_step(rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam, const float* d_half0,
                                const float* d_half1, const float* d_feat, float* d_out0, float* d_out1,
                                void* hip_stream) {
  return temporal_step<false, false>("rt_temporal_step", t, o, nullptr, cam, d_half0, d_half1, d_feat, nullptr, nullptr,
                                     0, d_out0, d_out1, hip_stream);
}

extern "C" int rt_temporal_step_motion(rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam,
                                       const float* d_half0, const float* d_half1, const float* d_feat,
                                       const int32_t* d_ids, const float* d_motion, int n_bodies, float* d_out0,
                                       float* d_out1, void* hip_stream) {
  return temporal_step<true, false>("rt_temporal_step_motion", t, o, nullptr, cam, d_half0, d_half1, d_feat, d_ids,
                                    d_motion, n_bodies, d_out0, d_out1, hip_stream);
}

// raytracing.clj:141-155's frames with the fetched history held to the current
// frame's colour box (rt.h); d_ids == NULL: rt_temporal_step's reprojection
extern "C" int rt_temporal_step_clamp(rt_temporal* t, const rt_temporal_opts* o, const rt_temporal_clamp_opts* k,
                                      const rt_camera* cam, const float* d_half0, const float* d_half1,
                                      const float* d_feat, const int32_t* d_ids, const float* d_motion, int n_bodies,
                                      float* d_out0, float* d_out1, void* hip_stream) {
  const std::string me("rt_temporal_step_clamp");
  if (!d_ids)
    return temporal_step<false, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, nullptr, nullptr, 0, d_out0, d_out1,
                                      hip_stream);
  return temporal_step<true, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, d_ids, d_motion, n_bodies, d_out0,
                                   d_out1, hip_stream);
}

extern "C" int rt_temporal_read(const rt_temporal* t, float* host_a0, float* host_a1, float* host_guide,
                                float* host_len, void* hip_stream) {
  clear_error();
  if (!t) return set_error(RT_E_ARG, "rt_temporal_read: NULL argument");
  std::lock_guard<std::mutex> lk(t->mu);
  HIP_TRY(hipSetDevice(t->device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device("rt_temporal_read", stream, t->device, "the history")) return rc;
  std::vector<TpWord> w0, w1;
  if (host_a0 || host_len) {
    w0.resize(t->n_px);
    HIP_TRY(hipMemcpyAsync(w0.data(), t->a0[t->cur].p, t->n_px * sizeof(TpWord), hipMemcpyDeviceToHost, stream));
  }
  if (host_a1) {
    w1.resize(t->n_px);
    HIP_TRY(hipMemcpyAsync(w1.data(), t->a1[t->cur].p, t->n_px * sizeof(TpWord), hipMemcpyDeviceToHost, stream));
  }
  if (host_guide)
    HIP_TRY(hipMemcpyAsync(host_guide, t->guide[t->cur].p, t->n_px * sizeof(DnGuide), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (size_t i = 0; i < t->n_px; ++i) {
    if (host_a0) {
      host_a0[3 * i] = w0[i].r;
      host_a0[3 * i + 1] = w0[i].g;
      host_a0[3 * i + 2] = w0[i].b;
    }
    if (host_len) host_len[i] = w0[i].l;
    if (host_a1) {
      host_a1[3 * i] = w1[i].r;
      host_a1[3 * i + 1] = w1[i].g;
      host_a1[3 * i + 2] = w1[i].b;
    }
  }
  return RT_OK;
}

// ---- the sample budget's steps (rt.h, temporal.h) ------------
// rt_temporal_step_budget: rt_temporal_step_clamp's step with the tiles'
// weights; gamma = +inf clamps nothing (rt.h), so no box is built then.
extern "C" int rt_temporal_step_budget(rt_temporal* t, const rt_temporal_opts* o, const rt_temporal_clamp_opts* k,
                                       const rt_camera* cam, const float* d_half0, const float* d_half1,
                                       const float* d_feat, const int32_t* d_ids, const float* d_motion, int n_bodies,
                                       const uint32_t* d_mult, float* d_out0, float* d_out1, void* hip_stream) {
  const std::string me("rt_temporal_step_budget");
  const bool box = !(k && k->gamma == INFINITY);
  if (!d_ids)
    return box ? temporal_step<false, true, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, nullptr, nullptr, 0, d_out0,
                                                  d_out1, hip_stream, d_mult)
               : temporal_step<false, false, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, nullptr, nullptr, 0,
                                                   d_out0, d_out1, hip_stream, d_mult);
  return box ? temporal_step<true, true, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, d_ids, d_motion, n_bodies,
                                               d_out0, d_out1, hip_stream, d_mult)
             : temporal_step<true, false, true>(me, t, o, k, cam, d_half0, d_half1, d_feat, d_ids, d_motion, n_bodies,
                                                d_out0, d_out1, hip_stream, d_mult);
}

// rt_temporal_probe: the step's checks and set-up, one kernel, no state touched
extern "C" int rt_temporal_probe(const rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam,
                                 const float* d_feat, const int32_t* d_ids, const float* d_motion, int n_bodies,
                                 float* d_len, void* hip_stream) {
  clear_error();
  const std::string me("rt_temporal_probe");
  if (!t || !cam || !d_feat || !d_len) return set_error(RT_E_ARG, me + ": NULL argument");
  const size_t lb = t->n_px * sizeof(float), fb = t->n_px * RT_FEAT_CHANNELS * sizeof(float);
  const size_t ib = d_ids ? t->n_px * sizeof(int32_t) : 0, mb = d_ids ? static_cast<size_t>(n_bodies) * 4 * sizeof(float) : 0;
  const TpSpan out{d_len, lb}, ins[] = {{d_feat, fb}, {d_ids, ib}, {d_motion, mb}};
  TpSetup s;
  if (const int rc = tp_set_up(me, t, o, nullptr, *cam, d_ids != nullptr, d_ids, d_motion, n_bodies, &out, 1, ins, 3,
                               hip_stream, &s))
    return rc;
  const TpFrame& f = s.f;
  const hipStream_t stream = s.stream;
  const dim3 grid = s.grid, block = s.block;
  const TpWord* a0 = t->a0[t->cur].p;
  const DnGuide* g = t->guide[t->cur].p;
  if (d_ids)
    HIP_TRY(enqueue(temporal_probe_kernel<true>, grid, block, 0, stream, f, d_feat, d_ids, d_motion, n_bodies, a0, g,
                    d_len));
  else
    HIP_TRY(enqueue(temporal_probe_kernel<false>, grid, block, 0, stream, f, d_feat, static_cast<const int32_t*>(nullptr),
                    static_cast<const float*>(nullptr), 0, a0, g, d_len));
  return RT_OK;
}

// ---- guided upsampling (rt.h, upsample.h) ---------------------
// rt_upsample: the checks, the device that holds d_out0, one kernel.
extern "C" int rt_upsample(const rt_upsample_opts* o, const float* d_half0, const float* d_half1,
                           const float* d_feat_coarse, const float* d_feat, int width, int rows, float* d_out0,
                           float* d_out1, void* hip_stream) {
  clear_error();
  const std::string me("rt_upsample");
  const rt_upsample_opts opt = o ? *o : up_default_opts();
  // (the kernel's grid has a block row per kDnBy image rows)
  if (rows > 65535 * kDnBy) return set_error(RT_E_ARG, me + ": bad width/rows");
  if (const char* why = up_args_error(opt, d_half0, d_half1, d_feat_coarse, d_feat, width, rows, d_out0, d_out1))
    return set_error(RT_E_ARG, me + ": " + why);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_error(RT_E_NODEV, me + ": no device available");
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, d_out0) != hipSuccess ||
      (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
    (void)hipGetLastError();
    return set_error(RT_E_ARG, me + ": d_out0 is not a device pointer");
  }
  const int device = at.device;
  HIP_TRY(hipSetDevice(device));
  const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (const int rc = stream_on_device(me, stream, device, "d_out0")) return rc;
  const dim3 grid(static_cast<unsigned>((width + kDnBx - 1) / kDnBx), static_cast<unsigned>((rows + kDnBy - 1) / kDnBy)),
      block(kDnBx, kDnBy);
  const bool two = d_half1 != nullptr;
  const auto fn = opt.scale == 2   ? (two ? upsample_kernel<2, true> : upsample_kernel<2, false>)
                  : opt.scale == 3 ? (two ? upsample_kernel<3, true> : upsample_kernel<3, false>)
                                   : (two ? upsample_kernel<4, true> : upsample_kernel<4, false>);
  HIP_TRY(enqueue(fn, grid, block, 0, stream, d_half0, d_half1, d_feat_coarse, d_feat, width, rows, opt.normal_pow2,
                  opt.sigma_z, d_out0, d_out1));
  return RT_OK;
}
