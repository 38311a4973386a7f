// rt_main — C++ host driver mirroring `clojure -M:main [spp] [depth]`
// (src/raytracing.clj:95-177): prints the config, renders the reference's
// five-body scene at 400x225 through rt_render, writes scene.ppm.
// --realm mirrors `clojure -M:realm` (src/realm/raytracing.clj:279-359)
// instead: realm's body order, camera (no defocus, focal length
// |look-from - look-at|), height (int (/ ^double 400 ^double 16/9)) = 224 and
// RT_FLAG_REALM semantics; it writes scene-realm.ppm.  Like the reference's
// -main, whose (time ...) ends with (ppm->png "scene.ppm" "scene.png")
// (raytracing.clj:176), it then converts the PPM it wrote to a PNG beside it
// (rt_ppm_to_png; --png PATH names it, --no-png skips it), inside the timing.  The frame
// is quantised on the device (rt_render_u8: a quarter of the copy back, no
// host pass); --host-quantize takes rt_render's floats and rt_quantize
// instead (the same bytes).
//
//   rt_main [spp] [depth] [--scene reference|cover] [--realm] [--width W]
//           [--seed S] [--gpus N] [--out PATH] [--png PATH] [--no-png] [--json]
//           [--host-quantize] [--rejection-samplers] [--passes K]
//           [--adaptive TOLQ16 [--step S] [--min-spp A] [--max-spp B]]
//           [--features STEM] [--denoise STEM [--scale N] [--chain K]]
// Defaults follow the reference: spp 100, depth 50, width 400, 16:9.
// --passes K: the spp in K near-equal accumulating passes on device 0
// (rt_launch_accum into an rt_accum, the sums read back, rt_resolve_sums and
// rt_quantize on the host): the same PPM / PNG bytes as without it.
// --adaptive TOLQ16: adaptive sampling on device 0 (rt_adapt: steps of S
// samples, default 10, until every 8 x 8 tile's two sample halves agree within
// TOLQ16 / 65536 after at least A samples, default 2 S, or holds B, default
// the spp argument); halves and counts are read back, rt_adapt_resolve_host
// and rt_quantize on the host.  Prints the samples traced and the tiles at
// the cap; --json carries them ("adaptive").
// --features STEM: after the render, the first-hit features of the frame's
// camera rays (rt_feat on device 0, the frame's spp and seed; include/rt.h):
// STEM.feat.f32 holds the resolved floats (rows x width x 8: albedo rgb,
// normal xyz, depth = the nearest hit, coverage; row-major, as the host
// stores them), STEM.albedo.png the albedo through rt_quantize,
// STEM.normal.png the bytes floor(255 * clamp(0.5 n + 0.5, 0, 1) + 0.5), linear.
// --denoise STEM: after the render, the frame once more on device 0 as two
// accumulators of spp / 2 samples each (sample indices [0, spp / 2) and
// [spp / 2, spp): the frame's own rays, at its seed) and the first-hit features
// of all spp, resolved on the device and filtered by rt_denoise with its
// default options (include/rt.h): STEM.denoised.ppm and STEM.denoised.png hold
// rt_quantize of the result.  An odd spp is an error (exit status 2).
// --scale N (2..4, with --denoise): the two accumulators and a second feature
// pass run on rt_camera_coarsen's camera at ceil(width / N) x ceil(height / N),
// spp samples per coarse pixel; rt_upsample (default options but the scale)
// brings the halves up to the frame's size through the frame's own features
// before rt_denoise.  Without --denoise, or outside 2..4: exit status 2.
// --chain K (0..64, with --denoise): the feature passes are specular-chain
// passes of at most K bounces (rt_launch_feat_chain, fuzz_max 0): the filter and
// --scale's upsampling are guided by what mirrors and glass show.  Without
// --denoise, or outside 0..64: exit status 2.
// --json: one more line, a JSON object of where this one-frame process's time
// went (the device start-up -- the HIP runtime's first rt_device_count, then
// rt_prepare's context / code object / queue / pageable staging -- on a thread
// beside the scene set-up, what the main thread waited for it; rt_render's
// rt_stats parts; quantise and file writes) -- bench.py's first_process.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <iterator>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>   // (--denoise's device frame: hipMalloc, hipMemcpy)

#include "../../include/rt.h"

int main(int argc, char** argv) {
  int spp = 100, depth = 50, width = 400, gpus = 0, grid = 11, passes = 0;
  int ad_step = 10, ad_min = 0, ad_max = 0;
  int scale = 0;   // --scale: the render scale of --denoise's frame (0: off)
  bool scale_given = false;
  int chain = -1;   // --chain: the bounces of --denoise's feature passes (< 0: first-hit features)
  bool chain_given = false;
  long long ad_tol = -1;   // --adaptive: the tolerance (< 0: off)
  long long ad_samples = 0;
  int ad_tiles = 0, ad_cap_tiles = 0, ad_steps = 0;
  unsigned long long seed = 1;
  std::string scene = "reference", out, png, features, denoise;
  bool realm = false, json = false, host_quantize = false, no_png = false, rejection = false;
  int pos = 0;
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  // The one-time device start-up first, on its own thread, while this one
  // parses the arguments and builds the scene: the HIP runtime (the first
  // rt_device_count), then per device its context, code object, queue and
  // pageable-copy staging (rt_prepare).
  int ndev = 0;
  double device_count_ms = 0.0, prep_ms[4] = {0, 0, 0, 0};
  int gpus_arg = 0;
  // (a missing option value ends the process before the start-up thread
  // exists: no exit while that thread may be inside the HIP runtime)
  static const char* const kValued[] = {"--scene", "--width", "--seed", "--gpus", "--grid", "--out", "--png", "--passes",
                                        "--adaptive", "--step", "--min-spp", "--max-spp", "--features", "--denoise",
                                        "--scale", "--chain"};
  for (int i = 1; i < argc; ++i) {
    const bool valued = std::any_of(std::begin(kValued), std::end(kValued),
                                    [&](const char* f) { return std::strcmp(argv[i], f) == 0; });
    if (!valued) continue;
    if (i + 1 >= argc) {
      std::fprintf(stderr, "missing value for %s\n", argv[i]);
      return 2;
    }
    if (std::strcmp(argv[i], "--gpus") == 0) gpus_arg = std::atoi(argv[i + 1]);
    ++i;
  }
  std::thread prep([&] {
    const auto t = std::chrono::steady_clock::now();
    ndev = rt_device_count();   // the process's first HIP call: runtime start-up
    device_count_ms = ms_since(t);
    const int use = gpus_arg > 0 ? std::min(gpus_arg, ndev) : ndev;
    std::vector<std::thread> per;
    std::vector<std::vector<double>> parts(use, std::vector<double>(4, 0.0));
    for (int d = 0; d < use; ++d) per.emplace_back([&, d] { rt_prepare(d, parts[d].data()); });
    for (auto& x : per) x.join();
    for (int d = 0; d < use; ++d)
      for (int k = 0; k < 4; ++k) prep_ms[k] = std::max(prep_ms[k], parts[d][k]);
  });
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> const char* { return argv[++i]; };   // (present: checked above)
    if (a == "--scene") scene = val();
    else if (a == "--width") width = std::atoi(val());
    else if (a == "--seed") seed = std::strtoull(val(), nullptr, 10);
    else if (a == "--gpus") gpus = std::atoi(val());
    else if (a == "--grid") grid = std::atoi(val());
    else if (a == "--out") out = val();
    else if (a == "--png") png = val();
    else if (a == "--passes") passes = std::atoi(val());
    else if (a == "--adaptive") ad_tol = std::atoll(val());
    else if (a == "--step") ad_step = std::atoi(val());
    else if (a == "--min-spp") ad_min = std::atoi(val());
    else if (a == "--max-spp") ad_max = std::atoi(val());
    else if (a == "--features") features = val();
    else if (a == "--denoise") denoise = val();
    else if (a == "--scale") scale = std::atoi(val()), scale_given = true;
    else if (a == "--chain") chain = std::atoi(val()), chain_given = true;
    else if (a == "--realm") realm = true;
    else if (a == "--rejection-samplers") rejection = true;   // RT_FLAG_REJECTION_SAMPLERS
    else if (a == "--json") json = true;
    else if (a == "--no-png") no_png = true;
    else if (a == "--host-quantize") host_quantize = true;
    else if (pos == 0) spp = std::atoi(argv[i]), ++pos;   // (:96)
    else if (pos == 1) depth = std::atoi(argv[i]), ++pos; // (:97)
  }
  if (out.empty()) out = realm ? "scene-realm.ppm" : "scene.ppm";
  if (png.empty() && !no_png) {   // scene.ppm -> scene.png (raytracing.clj:176)
    png = out;
    const size_t dot = png.rfind(".ppm");
    if (dot != std::string::npos && dot + 4 == png.size()) png.resize(dot);
    png += ".png";
  }
  if (no_png) png.clear();
  if (!realm) std::printf("config: {:samples-per-px %d, :max-depth %d}\n", spp, depth);  // (:98)
  // -main: (int (/ image-width 16/9)) in exact ratios (:105-107); realm: a
  // double division by Ratio.doubleValue(16/9) = 1.777777777777778
  // (realm/raytracing.clj:20-22), 400 -> 224
  const int height = realm ? static_cast<int>(width / 1.777777777777778) : width * 9 / 16;
  const int cap = RT_MAX_SPHERES;
  std::vector<float> sph(4 * cap), mat(4 * cap);
  std::vector<int> kind(cap);
  rt_camera cam{};
  int n = 0;
  if (scene == "cover") {
    n = rt_scene_cover(grid, 42, sph.data(), kind.data(), mat.data(), cap);
    const double lf[3] = {13, 2, 3}, la[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    rt_camera_setup(width, height, 20.0, lf, la, up, 0.6, 10.0, &cam);
  } else {
    n = rt_scene_reference(sph.data(), kind.data(), mat.data(), cap);
    const double lf[3] = {-2, 2, 1}, la[3] = {0, 0, -1}, up[3] = {0, 1, 0};  // (:110-115)
    if (realm) {
      // realm/raytracing.clj:307-317 lists the centre sphere before the ground
      for (int k = 0; k < 4; ++k) {
        std::swap(sph[k], sph[4 + k]);
        std::swap(mat[k], mat[4 + k]);
      }
      std::swap(kind[0], kind[1]);
      const double fl = std::sqrt(4.0 + 4.0 + 4.0);   // |look-from - look-at| (:291-292)
      rt_camera_setup(width, height, 20.0, lf, la, up, 0.0, fl, &cam);
    } else {
      rt_camera_setup(width, height, 20.0, lf, la, up, 10.0, 3.4, &cam);
    }
  }
  rt_scene s{n, sph.data(), kind.data(), mat.data()};
  const double scene_ms = ms_since(t_start);
  prep.join();   // (the device start-up ran beside the argument parsing and the scene)
  const double prep_wait_ms = ms_since(t_start) - scene_ms;
  if (!denoise.empty() && (spp <= 0 || spp % 2 != 0)) {
    std::fprintf(stderr, "--denoise needs an even spp (two halves of spp / 2 samples), got %d\n", spp);
    return 2;
  }
  if (scale_given && (denoise.empty() || scale < 2 || scale > 4)) {
    std::fprintf(stderr, "--scale needs --denoise and a value of 2..4, got %d\n", scale);
    return 2;
  }
  if (chain_given && (denoise.empty() || chain < 0 || chain > 64)) {
    std::fprintf(stderr, "--chain needs --denoise and a value of 0..64, got %d\n", chain);
    return 2;
  }
  rt_params p{};
  p.width = width;
  p.height = height;
  p.row_begin = 0;
  p.row_end = height;
  p.spp = spp;
  p.max_depth = depth;
  p.seed = seed;
  p.n_devices = gpus;
  p.flags = (realm ? RT_FLAG_REALM : 0) | (rejection ? RT_FLAG_REJECTION_SAMPLERS : 0);
  const auto t0 = std::chrono::steady_clock::now();
  const size_t nch = static_cast<size_t>(width) * height * 3;
  std::vector<uint8_t> q(nch);
  rt_stats st{};
  double render_ms = 0.0, quantize_ms = 0.0;
  if (ad_tol >= 0) {
    // compute-pixel's sample loop (raytracing.clj:141-155), tile by tile until
    // the tile's two halves agree
    rt_adapt_opts o{};
    o.step_spp = ad_step;
    o.min_spp = ad_min > 0 ? ad_min : 2 * ad_step;
    o.max_spp = ad_max > 0 ? ad_max : spp;
    o.tol_q16 = static_cast<uint32_t>(std::min<long long>(ad_tol, 0xffffffffll));
    rt_dscene* ds = nullptr;
    rt_adapt* ad = nullptr;
    bool ok = rt_scene_upload(0, &s, &ds) == RT_OK && rt_adapt_create(ds, &p, &o, &ad) == RT_OK;
    int traced = 1;
    while (ok && traced > 0) {
      traced = rt_adapt_step(ds, &cam, &p, ad, nullptr, nullptr);
      ok = traced >= 0;
      ad_steps += traced > 0;
    }
    ad_tiles = ((width + 7) / 8) * ((height + 7) / 8);
    std::vector<uint32_t> tile_spp(static_cast<size_t>(ad_tiles));
    ok = ok && rt_adapt_counts(ad, tile_spp.data(), nullptr) == RT_OK;
    std::vector<uint64_t> h0, h1;
    std::vector<float> lin;
    if (ok) {
      h0.resize(nch), h1.resize(nch), lin.resize(nch);
      ok = rt_adapt_read(ad, h0.data(), h1.data(), nullptr) == RT_OK &&
           rt_adapt_resolve_host(h0.data(), h1.data(), tile_spp.data(), width, height, p.flags, lin.data()) == RT_OK;
    }
    if (!ok) {
      std::fprintf(stderr, "--adaptive failed: %s\n", rt_last_error());
      return 1;
    }
    ad_samples = rt_adapt_samples(ad);
    for (uint32_t n : tile_spp) ad_cap_tiles += n >= static_cast<uint32_t>(o.max_spp);
    rt_adapt_free(ad);
    rt_scene_free(ds);
    render_ms = ms_since(t0);
    const auto t_q = std::chrono::steady_clock::now();
    rt_quantize(lin.data(), q.data(), q.size());
    quantize_ms = ms_since(t_q);
    st.n_devices = 1;
    st.samples = static_cast<uint64_t>(ad_samples);
  } else if (passes > 0) {
    // compute-pixel's sample loop (raytracing.clj:141-155) in K launches
    rt_dscene* ds = nullptr;
    rt_accum* acc = nullptr;
    std::vector<uint64_t> sums(nch);
    std::vector<float> lin(nch);
    const int k = std::max(1, std::min(passes, std::max(spp, 1)));
    bool ok = rt_scene_upload(0, &s, &ds) == RT_OK && rt_accum_create(ds, &p, &acc) == RT_OK;
    rt_params pp = p;
    for (int i = 0; ok && i < k; ++i) {
      pp.spp = spp / k + (i < spp % k ? 1 : 0);
      ok = rt_launch_accum(ds, &cam, &pp, acc, nullptr, nullptr) == RT_OK;
      pp.sample_begin += pp.spp;
    }
    ok = ok && rt_accum_read(acc, sums.data(), nullptr) == RT_OK &&
         rt_resolve_sums(sums.data(), sums.size(), rt_accum_samples(acc), p.flags, lin.data()) == RT_OK;
    if (!ok) {
      std::fprintf(stderr, "--passes failed: %s\n", rt_last_error());
      return 1;
    }
    rt_accum_free(acc);
    rt_scene_free(ds);
    render_ms = ms_since(t0);
    const auto t_q = std::chrono::steady_clock::now();
    rt_quantize(lin.data(), q.data(), q.size());
    quantize_ms = ms_since(t_q);
    st.n_devices = 1;
    st.samples = static_cast<uint64_t>(width) * height * static_cast<uint64_t>(std::max(spp, 0));
  } else if (host_quantize) {
    std::vector<float> lin(nch);
    if (rt_render(&s, &cam, &p, lin.data(), lin.size(), &st) != RT_OK) {
      std::fprintf(stderr, "rt_render failed: %s\n", rt_last_error());
      return 1;
    }
    render_ms = ms_since(t0);
    const auto t_q = std::chrono::steady_clock::now();
    rt_quantize(lin.data(), q.data(), q.size());
    quantize_ms = ms_since(t_q);
  } else {
    if (rt_render_u8(&s, &cam, &p, q.data(), q.size(), &st) != RT_OK) {
      std::fprintf(stderr, "rt_render_u8 failed: %s\n", rt_last_error());
      return 1;
    }
    render_ms = ms_since(t0);
  }
  const auto t_w = std::chrono::steady_clock::now();
  if (rt_write_ppm(out.c_str(), q.data(), width, height) != RT_OK) {
    std::fprintf(stderr, "%s\n", rt_last_error());
    return 1;
  }
  const double write_ms = ms_since(t_w);
  // (ppm->png "scene.ppm" "scene.png"): the reference reads the PPM it wrote
  // back and encodes it (ppm2png.clj:35-87); so does this, inside the timing
  const auto t_p = std::chrono::steady_clock::now();
  if (!png.empty() && rt_ppm_to_png(out.c_str(), png.c_str()) != RT_OK) {
    std::fprintf(stderr, "%s\n", rt_last_error());
    return 1;
  }
  const double png_ms = png.empty() ? 0.0 : ms_since(t_p);
  if (!features.empty()) {
    // the features of the rays the frame traced (raytracing.clj:144-151, :33-43)
    const size_t npx = static_cast<size_t>(width) * height;
    rt_dscene* ds = nullptr;
    rt_feat* ft = nullptr;
    std::vector<int64_t> sums(npx * 6);
    std::vector<uint32_t> hits(npx);
    std::vector<float> fdepth(npx), feat(npx * RT_FEAT_CHANNELS), alb(npx * 3);
    std::vector<uint8_t> b8(npx * 3);
    bool ok = rt_scene_upload(0, &s, &ds) == RT_OK && rt_feat_create(ds, &p, &ft) == RT_OK &&
              rt_launch_feat(ds, &cam, &p, ft, nullptr, nullptr) == RT_OK &&
              rt_feat_read(ft, sums.data(), hits.data(), fdepth.data(), nullptr) == RT_OK &&
              rt_feat_resolve_host(sums.data(), hits.data(), fdepth.data(), npx, rt_feat_samples(ft), feat.data()) == RT_OK;
    if (ok) {
      FILE* f = std::fopen((features + ".feat.f32").c_str(), "wb");
      ok = f && std::fwrite(feat.data(), sizeof(float), feat.size(), f) == feat.size();
      if (f) ok = std::fclose(f) == 0 && ok;
      if (!ok) std::fprintf(stderr, "cannot write %s.feat.f32\n", features.c_str());
    } else {
      std::fprintf(stderr, "--features failed: %s\n", rt_last_error());
    }
    if (ok) {
      for (size_t i = 0; i < npx; ++i)
        for (int c = 0; c < 3; ++c) alb[3 * i + c] = feat[RT_FEAT_CHANNELS * i + c];
      ok = rt_quantize(alb.data(), b8.data(), b8.size()) == RT_OK &&
           rt_write_png((features + ".albedo.png").c_str(), b8.data(), width, height) == RT_OK;
      for (size_t i = 0; i < npx; ++i)
        for (int c = 0; c < 3; ++c) {
          const double v = 0.5 * static_cast<double>(feat[RT_FEAT_CHANNELS * i + 3 + c]) + 0.5;   // (the product is exact)
          const double cl = v > 0.0 ? (v < 1.0 ? v : 1.0) : 0.0;
          const double sc = cl * 255.0;
          b8[3 * i + c] = static_cast<uint8_t>(std::floor(sc + 0.5));
        }
      ok = ok && rt_write_png((features + ".normal.png").c_str(), b8.data(), width, height) == RT_OK;
      if (!ok) std::fprintf(stderr, "%s\n", rt_last_error());
    }
    rt_feat_free(ft);
    rt_scene_free(ds);
    if (!ok) return 1;
  }
  if (!denoise.empty()) {
    // the frame's rays as two halves and their features (raytracing.clj:141-155,
    // :144-151, :33-43), resolved and filtered on device 0
    // (--scale: the halves and a second feature pass on the coarsened camera,
    // :129-135, brought up to the frame's size by rt_upsample)
    const size_t npx = static_cast<size_t>(width) * height;
    rt_dscene* ds = nullptr;
    rt_accum* acc[2] = {nullptr, nullptr};
    rt_feat *ft = nullptr, *fc = nullptr;
    rt_denoiser* dn = nullptr;
    // half0 | half1 | out (3 floats a pixel each) | feat (8); with --scale then
    // the coarse half0 | half1 (3 a coarse pixel each) | the coarse feat (8)
    float* d_buf = nullptr;
    std::vector<float> lin(npx * 3);
    std::vector<uint8_t> b8(npx * 3);
    rt_params hp = p;
    rt_camera hcam = cam;
    if (scale) {
      hp.width = (width + scale - 1) / scale;
      hp.height = hp.row_end = (height + scale - 1) / scale;
    }
    const size_t ncp = scale ? static_cast<size_t>(hp.width) * hp.height : 0;
    rt_params cp = hp;   // the coarse frame's feature pass: all spp
    cp.n_devices = 0;
    hp.n_devices = 0;
    hp.spp = spp / 2;
    bool ok = rt_scene_upload(0, &s, &ds) == RT_OK && rt_feat_create(ds, &p, &ft) == RT_OK &&
              rt_denoiser_create(0, width, height, &dn) == RT_OK &&
              (!scale || (rt_camera_coarsen(&cam, scale, &hcam) == RT_OK && rt_feat_create(ds, &cp, &fc) == RT_OK));
    for (int k = 0; ok && k < 2; ++k) {
      hp.sample_begin = k * (spp / 2);
      ok = rt_accum_create(ds, &hp, &acc[k]) == RT_OK && rt_launch_accum(ds, &hcam, &hp, acc[k], nullptr, nullptr) == RT_OK;
    }
    // (--chain: the guides of what mirrors and glass show, raytracing.clj:45-58)
    const rt_feat_chain_opts co{chain, 0.0f};
    auto feat_pass = [&](const rt_camera* fcam, const rt_params* fp, rt_feat* f) {
      return chain_given ? rt_launch_feat_chain(ds, fcam, fp, &co, f, nullptr, nullptr)
                         : rt_launch_feat(ds, fcam, fp, f, nullptr, nullptr);
    };
    ok = ok && feat_pass(&cam, &p, ft) == RT_OK && (!scale || feat_pass(&hcam, &cp, fc) == RT_OK);
    if (!ok) std::fprintf(stderr, "--denoise failed: %s\n", rt_last_error());
    if (ok && hipMalloc(reinterpret_cast<void**>(&d_buf),
                        (npx * (9 + RT_FEAT_CHANNELS) + ncp * (6 + RT_FEAT_CHANNELS)) * sizeof(float)) != hipSuccess) {
      std::fprintf(stderr, "--denoise failed: no device memory for the frame\n");
      ok = false;
    }
    if (ok) {
      float *d_h0 = d_buf, *d_h1 = d_buf + npx * 3, *d_out = d_buf + npx * 6, *d_feat = d_buf + npx * 9;
      float *d_c0 = d_feat + npx * RT_FEAT_CHANNELS, *d_c1 = d_c0 + ncp * 3, *d_fc = d_c1 + ncp * 3;
      rt_upsample_opts uo{scale, 0, 0.05f};   // (rt.h's defaults but the scale)
      ok = rt_accum_resolve(acc[0], p.flags, scale ? d_c0 : d_h0, nullptr) == RT_OK &&
           rt_accum_resolve(acc[1], p.flags, scale ? d_c1 : d_h1, nullptr) == RT_OK &&
           rt_feat_resolve(ft, d_feat, nullptr) == RT_OK &&
           (!scale || (rt_feat_resolve(fc, d_fc, nullptr) == RT_OK &&
                       rt_upsample(&uo, d_c0, d_c1, d_fc, d_feat, width, height, d_h0, d_h1, nullptr) == RT_OK)) &&
           rt_denoise(dn, nullptr, d_h0, d_h1, d_feat, d_out, nullptr) == RT_OK;
      if (!ok) std::fprintf(stderr, "--denoise failed: %s\n", rt_last_error());
      if (ok && hipMemcpy(lin.data(), d_out, lin.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "--denoise failed: the copy back\n");
        ok = false;
      }
    }
    if (ok) {
      ok = rt_quantize(lin.data(), b8.data(), b8.size()) == RT_OK &&
           rt_write_ppm((denoise + ".denoised.ppm").c_str(), b8.data(), width, height) == RT_OK &&
           rt_write_png((denoise + ".denoised.png").c_str(), b8.data(), width, height) == RT_OK;
      if (!ok) std::fprintf(stderr, "%s\n", rt_last_error());
    }
    if (d_buf) (void)hipFree(d_buf);
    rt_denoiser_free(dn);
    rt_feat_free(ft);
    rt_feat_free(fc);
    rt_accum_free(acc[0]);
    rt_accum_free(acc[1]);
    rt_scene_free(ds);
    if (!ok) return 1;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::printf("\"Elapsed time: %.3f msecs\"\n", ms);  // (time ...) (:99)
  if (ad_tol >= 0)
    std::printf("bodies %d, devices 1, adaptive: %d steps, %lld samples traced of %lld at the cap, %d of %d tiles at "
                "the cap, %.3f ms\n", n, ad_steps, ad_samples,
                static_cast<long long>(width) * height * (ad_max > 0 ? ad_max : spp), ad_cap_tiles, ad_tiles, render_ms);
  else if (passes > 0)
    std::printf("bodies %d, devices 1, %d passes, %.3f ms, %.1f Msamples/s\n", n,
                std::max(1, std::min(passes, std::max(spp, 1))), render_ms, st.samples / (render_ms * 1e3));
  else
    std::printf("bodies %d, devices %d, kernel %.3f ms, %.1f Msamples/s, %.3f segments/sample\n", n,
                st.n_devices, st.kernel_ms, st.samples / (st.kernel_ms * 1e3),
                st.samples ? double(st.segments) / st.samples : 0.0);
  if (json)
    std::printf(
        "{\"devices_visible\": %d, \"scene_ms\": %.3f, \"device_count_ms\": %.3f, \"prepare_ms\": {\"context\": %.3f, "
        "\"code_object\": %.3f, \"queue\": %.3f, \"pageable_staging\": %.3f}, \"prepare_wait_ms\": %.3f, "
        "\"render_ms\": %.3f, \"quantize\": \"%s\", "
        "\"quantize_ms\": %.3f, \"write_ms\": %.3f, \"png_ms\": %.3f, \"process_ms\": %.3f, \"rt_stats\": {\"total_ms\": %.3f, "
        "\"upload_ms\": %.3f, \"setup_ms\": %.3f, \"enqueue_ms\": %.3f, \"wait_ms\": %.3f, \"scatter_ms\": %.3f, "
        "\"other_ms\": %.3f, \"kernel_ms\": %.3f, \"d2h_ms\": %.3f, \"segments\": %llu, \"samples\": %llu, "
        "\"n_devices\": %d}, \"adaptive\": {\"on\": %d, \"steps\": %d, \"samples_traced\": %lld, "
        "\"tiles\": %d, \"tiles_at_cap\": %d}}\n",
        ndev, scene_ms, device_count_ms, prep_ms[0], prep_ms[1], prep_ms[2], prep_ms[3], prep_wait_ms, render_ms,
        (host_quantize || passes > 0 || ad_tol >= 0) ? "host" : "device", quantize_ms, write_ms, png_ms, ms_since(t_start), st.total_ms,
        st.upload_ms, st.setup_ms, st.enqueue_ms, st.wait_ms, st.scatter_ms, st.other_ms, st.kernel_ms, st.d2h_ms,
        static_cast<unsigned long long>(st.segments), static_cast<unsigned long long>(st.samples), st.n_devices,
        ad_tol >= 0 ? 1 : 0, ad_steps, ad_samples, ad_tiles, ad_cap_tiles);
  return 0;
}
