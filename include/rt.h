/*
 * rt.h — C ABI of the MI355X-native per-pixel render loop.
 *
 * This is the drop-in boundary for the reference's hot path
 * (keychera/raytracing-clj, Clojure, no FFI of its own). It replaces:
 *
 *   compute-pixel + the row-chunk executor   src/raytracing.clj:141-171
 *     └ ray-color (recursive bounce)         src/raytracing.clj:45-58
 *        └ hit-anything (closest-hit scan)   src/raytracing.clj:33-43
 *           └ sphere ::hit-fn                src/hittable.clj:7-31
 *        └ material ::scatter-fn             src/material.clj:13-46
 *           (lambertian :13-19, metal :21-28, dielectric :34-46)
 *        └ vec3a math + rand samplers        src/vec3a.clj:56-101
 *
 * Scene definition (raytracing.clj:63-78), camera set-up (:101-139) and the
 * PPM writer (:19-26, :172-175) stay on the host; helpers for them are
 * exported here too (rt_camera_setup, rt_quantize, rt_write_ppm) so a
 * Clojure/JNI, C++ or Python host can reuse them.
 *
 * Conventions: plain pointers and sizes, no ownership transfer (the library
 * never retains a caller pointer past the call), 0 = OK, negative = error
 * (see rt_status; message via rt_last_error(), thread-local).
 */
#ifndef RT_H
#define RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the functions
 * declared here are exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ABI revision of this header (rt_abi_version() of the loaded library must
 * equal it; INTEGRATION.md lists the breaks).  3: rt_stats grew to 112 bytes
 * (set-up/enqueue/wait/scatter/other/D2H timers). */
#define RT_ABI_VERSION 3

/* ---- status codes ------------------------------------------------------ */
typedef enum rt_status {
  RT_OK = 0,
  RT_E_ARG = -1,        /* bad argument (NULL, size, range)                      */
  RT_E_MATERIAL = -2,   /* unsupported material kind                             */
  RT_E_TOO_MANY = -3,   /* sphere list larger than the LDS-resident limit        */
  RT_E_HIP = -4,        /* HIP runtime error (message has the HIP error string)  */
  RT_E_NODEV = -5,      /* no GPU visible / device index out of range            */
  RT_E_IO = -6,         /* file I/O (rt_write_ppm, rt_write_png, rt_ppm_to_png)  */
  RT_E_ALLOC = -7       /* host memory exhausted (the JNI shim's frame buffer)   */
} rt_status;

/* ---- material kinds: material.clj:13 (lambertian), :21 (metal), :34 (dielectric).
 * RT_NONE: a body merged with no material: ray-color finds no scatter-fn and
 * returns black (raytracing.clj:49-54). */
enum { RT_LAMBERTIAN = 0, RT_METAL = 1, RT_DIELECTRIC = 2, RT_NONE = 3 };

/* Maximum spheres per scene (LDS-resident sphere table, 16 B each). */
#define RT_MAX_SPHERES 8192

/* Maximum samples per pixel of one call (the pixel's fixed-point colour sums,
 * 2^-24 units per sample, stay below 2^64; larger counts: several passes with
 * sample_begin into an rt_accum, below, which adds them up exactly, to
 * 2^32 - 1 samples per pixel).  A sample's colour channel enters that sum clamped to
 * [0, 256): a negative or NaN channel counts as 0 (the Clojure code would sum
 * it), one of 256 or more as 256 - 2^-24. */
#define RT_MAX_SPP (1 << 24)

/* ---- scene: the reference's `hittables` vector (raytracing.clj:63-78) -----
 * Bodies are tested in array order; on equal t the earlier body wins, exactly
 * as hit-anything's strict `root < closest-so-far` (raytracing.clj:35-42,
 * hittable.clj:17-23); identical spheres are such ties, in every kernel
 * variant.
 *
 * What the arrays may hold beyond the reference's own scenes
 * (tests/test_gpu_input_edges.py pins each against the fp32 mirror, and
 * against the fp64 reference semantics where the two mean the same):
 *  - Albedos above 1 are accepted; a scene with one runs the kernel with
 *    64-bit pixel sums (rt_set_variant: 16 instead of 22).  Albedos below 0
 *    and sample colours of 256 or more meet the clamp described at
 *    RT_MAX_SPP.
 *  - Fuzz and refraction index are used as given, whatever their value
 *    (fuzz above 1 or below 0; an index of 1, below 1, negative, 0 or
 *    infinite): 1 / index and Schlick's r0 may then be infinite or NaN.  For
 *    the values named the frames stay the fp64 path's; under RT_FLAG_REALM
 *    an infinite index gives the same colours in more segments (a NaN
 *    product reflects here and refracts there).
 *  - A negative radius gives the inward normal, as hittable.clj:25's division
 *    by the radius does (a bubble inside glass as r < 0).
 *  - A body with a NaN or infinite coordinate or radius, or with a radius of
 *    2^64 or more (r * r overflows), is never hit; r = 0 neither, in
 *    practice.  This differs from the Clojure comparisons, which let a NaN
 *    root through.
 *  - Coordinates: scene and camera may be scaled together from 2^-62 to 2^20
 *    of unit scale with the fp64 meaning kept (the denormal range of r * r
 *    included; below 2^-40 a bounced ray's t > 1e-3, which is absolute in
 *    the reference too, ends every path at its second segment).  From 2^40
 *    the fp32 range and that absolute 1e-3 give out: the frame stays finite
 *    and equal across kernel variants, but no longer means what the fp64
 *    path computes. */
typedef struct rt_scene {
  int n;                  /* number of bodies                                  */
  const float* sphere;    /* n x 4: center x,y,z, radius  (hittable.clj:7)     */
  const int* mat_kind;    /* n: RT_LAMBERTIAN | RT_METAL | RT_DIELECTRIC | RT_NONE */
  const float* mat;       /* n x 4: albedo r,g,b, then fuzz (metal) or
                             refraction index (dielectric); unused lanes 0     */
} rt_scene;

/* ---- camera: the values -main derives at raytracing.clj:117-139 ---------- */
typedef struct rt_camera {
  float center[3];        /* camera-center = look-from          (:126)          */
  float p00[3];           /* pixel-00-loc                       (:135)          */
  float du[3];            /* pixel-du                           (:129)          */
  float dv[3];            /* pixel-dv                           (:130)          */
  float disk_u[3];        /* defocus-disk-u                     (:138)          */
  float disk_v[3];        /* defocus-disk-v                     (:139)          */
  int defocus;            /* defocus-angle > 0                  (:147)          */
} rt_camera;

/* ---- render parameters -----------------------------------------------------
 * Pixel (i, j) of sample k gets its own RNG stream keyed by (seed, j*width+i,
 * sample_begin+k): results do not depend on tiling, device count or launch
 * shape.  spp / max_depth are the reference's CLI args (raytracing.clj:96-97).
 *
 * Output rows: the rendered rows are [row_begin, row_end).  With
 * tile_step == 0 they are written contiguously.  With tile_step > 0 the call
 * renders only the interleaved row tiles  tile_first, tile_first+tile_step,
 * ... (tile height row_tile, tiles counted from row_begin) and writes them
 * compacted, in order; rt_rows_out() gives the row count. */
typedef struct rt_params {
  int width, height;      /* full image; height = int(width/aspect) (:105-107) */
  int row_begin, row_end; /* global rows to render                             */
  int spp;                /* samples per pixel in this call                    */
  int max_depth;          /* ray-color depth budget                            */
  uint64_t seed;          /* RNG key                                           */
  int sample_begin;       /* first sample index (sample stripes), usually 0    */
  int n_devices;          /* rt_render fan-out: 0 = all visible devices        */
  int row_tile;           /* interleaved tile height (rows); 0 -> 8            */
  int tile_first;         /* rt_launch: first tile of this shard               */
  int tile_step;          /* rt_launch: tile stride (0 = contiguous rows)      */
  int flags;              /* 0, RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS,
                             RT_FLAG_SHARDS_ON_DEVICE0 (rt_render),
                             RT_FLAG_STREAMED (rt_launch), ored                 */
} rt_params;

/* rt_render: split into n_devices interleaved-tile shards exactly as for n
 * GPUs, but run every shard on device 0 (exercises the multi-GPU fan-out and
 * host gather on a one-GPU machine).  n_devices must be > 0. */
#define RT_FLAG_SHARDS_ON_DEVICE0 1

/* rt_launch / rt_render: the semantics of the reference's second namespace,
 * realm.raytracing (`clojure -M:realm`, src/realm/raytracing.clj) instead of
 * raytracing (`-M:main`): lambertian scatter without the near-zero fallback
 * (:137-143), dielectric without Schlick reflectance and its draw (:158-177),
 * and the pixel as sum * (1/spp) rather than sum / spp (:25, :276).  Its
 * camera (no defocus, focal length |lookfrom - lookat|) is an rt_camera like
 * any other (rt_camera_setup with defocus_angle 0). */
#define RT_FLAG_REALM 2

/* rt_launch only: the caller keeps launches of consecutive frames in flight
 * on two (or more) streams of the device, so the next frame's workgroups fill
 * the slots this launch's tail frees.  A launch of few tiles then splits its
 * tiles' samples for two rounds of workgroups instead of three (fewer, longer
 * sample pools: each pool's end idles lanes; the tail no longer waits alone).
 * Timing only: the bits never depend on it.  (tools/shard_time.py
 * --inflight; bench.py's frames in flight) */
#define RT_FLAG_STREAMED 4

/* rt_launch / rt_render: draw vec3a/random-unit-vec3 and random-in-unit-disk
 * by the reference's own rejection loops (vec3a.clj:74-86: three or two
 * uniforms per trip until the point falls inside the unit ball / disk).
 * Without the flag (the default) the kernel draws the same distributions
 * with a fixed number of draws -- uniform on the sphere as z = 2 xi1 - 1,
 * r = sqrt(1 - z^2), at the angle 2 pi xi2; uniform in the disk as
 * r = sqrt(xi1) at 2 pi xi2 -- so a wave no longer waits for its slowest
 * lane's rejection trips (C1 5.23 -> 4.75 ms per frame).
 * The reference's rand is unseeded, so either choice matches its renders
 * statistically (tests/test_oracle_pinning.py); each equals its own fp32
 * mirror in the oracle bit for bit.  Mixed within one frame never. */
#define RT_FLAG_REJECTION_SAMPLERS 8

/* ---- per-call statistics (device-side counters, host timers) ------------ */
typedef struct rt_stats {
  uint64_t segments;      /* hit-anything calls (raytracing.clj:48)            */
  uint64_t samples;       /* compute-pixel loop iterations (:142-154)          */
  double kernel_ms;       /* max over devices of the trace-kernel time         */
  double total_ms;        /* wall time of the whole call incl. H2D/D2H         */
  int n_devices;          /* devices used                                      */
  int scene_cached;       /* devices whose scene came from the library's cache */
  double upload_ms;       /* max over devices: the wait for the scene's upload +
                             BVH builds (a cache miss; they run beside the
                             render-context set-up, this is what is left)      */
  double gather_ms;       /* max over devices: D2H of the device's row tiles
                             into their rows of out_rgb (strided copies)       */
  double kernel_ms_mean;  /* mean over devices of the trace-kernel time
                             (load imbalance = kernel_ms / kernel_ms_mean)     */
  /* Where the wall time of the slowest device's share went (host clocks, in
   * order): setup_ms, upload_ms above, then the others; the rest of total_ms
   * (argument checks, thread fan-out and join) is other_ms.  A first call
   * shows its one-time costs here: setup_ms (events, device framebuffer,
   * pinned counters; a device's first context runs on its NULL stream, a
   * created stream costs 5-7 ms), upload_ms (what the scene upload and BVH
   * builds add beyond the set-up they run beside) and enqueue_ms (the first
   * launch loads the kernels' code object).                                  */
  double setup_ms;        /* render context set-up                             */
  double enqueue_ms;      /* rt_launch + D2H enqueue                           */
  double wait_ms;         /* host wait for the device: kernel + D2H            */
  double scatter_ms;      /* host scatter of row tiles: 0 since ABI 3's
                             strided copies place the rows                    */
  double other_ms;        /* total_ms - upload - setup - enqueue - wait - scatter */
  double d2h_ms;          /* max over devices: event-timed D2H of the frame    */
} rt_stats;

/* ========================= host-side helpers =========================== */

/* Camera basis exactly as -main computes it, in double, rounded to float at
 * the end (raytracing.clj:105-139; deg->rad :60-61).  vfov/defocus_angle in
 * degrees.  Viewport width uses image_width/image_height, not the aspect
 * ratio (:120). */
int rt_camera_setup(int image_width, int image_height, double vfov,
                    const double look_from[3], const double look_at[3],
                    const double vup[3], double defocus_angle,
                    double focus_dist, rt_camera* out);

/* The camera of a frame of ceil(width / scale) x ceil(height / scale) pixels
 * whose pixel (I, J) covers the pixels [scale I, scale I + scale) x [scale J,
 * scale J + scale) of c's frame -- raytracing.clj:129-135's pixel deltas and
 * pixel00-loc for a viewport divided scale times more coarsely.  In double
 * from c's float fields, each component rounded to float once:
 *   p00' = p00 + ((scale - 1) / 2) * (du + dv),  du' = scale * du,  dv' = scale * dv;
 * center, disk_u, disk_v and defocus are copied.  A pixel's sample is
 * p00 + fx du + fy dv with the jitter in fx, fy, so a sample of the coarse
 * frame falls uniformly over its whole block.  scale is 2..4, else RT_E_ARG
 * (as is a NULL argument); out may be c.  rt_upsample brings such a frame back
 * to c's size. */
int rt_camera_coarsen(const rt_camera* c, int scale, rt_camera* out);

/* write-color! per channel (raytracing.clj:19-26):
 * out = int(256 * clamp(c > 0 ? sqrt(c) : 0, 0, 0.999)); NaN -> 0.  n = channel count. */
int rt_quantize(const float* lin, uint8_t* out, size_t n);

/* PPM P3, one "r g b\n" per pixel, rows top->bottom (raytracing.clj:172-175). */
int rt_write_ppm(const char* path, const uint8_t* rgb, int width, int height);

/* PNG, 8-bit truecolour RGB, adaptive per-row filters, deflate: the same
 * pixels as rt_write_ppm (the format src/ppm2png.clj:35-87 converts to). */
int rt_write_png(const char* path, const uint8_t* rgb, int width, int height);

/* ppm->png (src/ppm2png.clj:35-87): read a P3 file (max value <= 255, w*h
 * pixels of 3 values) and write it as rt_write_png does.  RT_E_ARG on a
 * malformed PPM, RT_E_IO on file errors. */
int rt_ppm_to_png(const char* src_ppm, const char* dst_png);

/* Number of output rows a (row_begin,row_end,row_tile,tile_first,tile_step)
 * selection produces (0 on bad args). */
int rt_rows_out(const rt_params* p);

/* ---- scene builders (host) ----------------------------------------------
 * Both write up to `cap` bodies into sphere (x4), kind, mat (x4) and return
 * the body count (the needed count when the arrays are NULL / cap too small).
 *
 * rt_scene_reference: the reference's five bodies, in order
 *   (raytracing.clj:63-78): ground, center, left (glass), bubble, right (metal).
 * rt_scene_cover: the RTIOW "final render" cover scene (book §14; the
 *   reference has no such scene): ground r=1000, a
 *   (2*grid)^2 jittered field of r=0.2 bodies (80 % lambertian, 15 % metal,
 *   5 % glass; skipped within 0.9 of (4,0.2,0)), then three r=1 bodies.
 *   Deterministic in `seed` (splitmix64 stream, 53-bit doubles). */
int rt_scene_reference(float* sphere, int* kind, float* mat, int cap);
int rt_scene_cover(int grid, uint64_t seed, float* sphere, int* kind, float* mat, int cap);

/* ============================ rendering ================================ */

/* Render into a caller-owned host buffer of linear RGB fp32, row-major,
 * rows_out x width x 3, the mean over spp (compute-pixel's accum/spp,
 * raytracing.clj:155).  Fans out over p->n_devices GPUs inside the call
 * (a host worker per device from a persistent pool, interleaved row tiles,
 * each device's rows copied straight into their place; no collectives).  tile_first/tile_step must be 0 here.  stats may be NULL.
 *
 * The device copy of the scene (tables + BVHs) is cached per device by the
 * scene's content (a hash, then a byte compare): a repeated call with the
 * same bodies skips the upload and the BVH builds, and its launches reuse
 * the per-device stream whose adaptive tile order (rt_set_schedule) the
 * previous call recorded.  The library keeps copies, never caller pointers.
 * Output bits never depend on the cache. */
int rt_render(const rt_scene* s, const rt_camera* c, const rt_params* p,
              float* out_rgb, size_t out_len, rt_stats* stats);

/* rt_render, then rt_quantize on the device: out_rgb8 (rows_out x width x 3
 * bytes) holds exactly the bytes rt_quantize gives for rt_render's floats,
 * the write-color! bytes of the -main loop (raytracing.clj:160-175), at a
 * quarter of the copy back.  stats->d2h_ms includes the quantiser. */
int rt_render_u8(const rt_scene* s, const rt_camera* c, const rt_params* p,
                 uint8_t* out_rgb8, size_t out_len, rt_stats* stats);

/* ---- frames in flight: a host drawing a sequence of frames ---------------
 * rt_render_submit starts the frame rt_render would render -- the same
 * shards, scene cache, devices and bits -- and returns without waiting for
 * the devices; rt_render_wait blocks until the frame's rows are in out_rgb
 * (which the caller leaves alone until then), fills stats as rt_render does
 * and frees the frame.  Frames submitted before earlier ones are waited on
 * run concurrently: each frame in flight holds its own render context
 * (stream, device buffers) per device, and its launches split their tiles'
 * samples for two rounds of workgroups (RT_FLAG_STREAMED), so the next
 * frame's workgroups fill this one's tail.  Every submitted frame must be
 * waited on exactly once, from any thread.  (raytracing.clj:157-171's
 * executor hands its futures back the same way: submit, then .get in order.)
 * The _u8 form delivers rt_render_u8's bytes. */
typedef struct rt_frame rt_frame;
int rt_render_submit(const rt_scene* s, const rt_camera* c, const rt_params* p, float* out_rgb,
                     size_t out_len, rt_frame** frame);
int rt_render_submit_u8(const rt_scene* s, const rt_camera* c, const rt_params* p, uint8_t* out_rgb8,
                        size_t out_len, rt_frame** frame);
int rt_render_wait(rt_frame* frame, rt_stats* stats);

/* Drop rt_render's cached device scenes and render contexts (streams,
 * buffers; those not in use by a concurrent call).  Returns the number of
 * scenes dropped. */
int rt_cache_clear(void);

/* Device-resident path (inputs already in HBM; used by the benchmark). */
typedef struct rt_dscene rt_dscene;
int rt_scene_upload(int device, const rt_scene* s, rt_dscene** out);
int rt_scene_free(rt_dscene* ds);
/* Asynchronous: enqueue one trace launch on hip_stream (NULL = default
 * stream) of ds's device.  d_out: device buffer of rt_rows_out(p) x width x 3
 * floats.  d_counters: NULL or device u64[2] += {segments, samples}.
 * A launch of fewer 8 x 8 tiles than 3 x the workgroups the device holds at
 * once (a multi-GPU shard, a small frame) splits every tile's samples over
 * several workgroups; their integer pixel sums are added by a second kernel
 * on the same stream, from a scratch buffer the library keeps per scene and
 * stream (splits x rows x width x 3 x 8 bytes).  Bits never depend on it. */
int rt_launch(const rt_dscene* ds, const rt_camera* c, const rt_params* p,
              float* d_out, uint64_t* d_counters, void* hip_stream);

/* ---- progressive rendering: samples accumulated on the device -------------
 * compute-pixel's loop over the samples of a pixel (raytracing.clj:141-155)
 * continued across launches.  A pixel is an integer sum of its samples'
 * colours in 2^-24 units, whatever the order; an rt_accum keeps those sums
 * (rt_rows_out(shape) x width x 3 u64, on the scene's device, zeroed by the
 * library) and the samples per pixel they hold, so that k passes of a frame
 * are, bit for bit, the frame one rt_launch of the total spp gives -- for
 * any pass sizes, launch shapes, order, streams or devices.
 *
 * rt_accum_create (raytracing.clj:141-155): an empty accumulator for frames
 * of `shape`'s width, height and row selection (row_begin, row_end, row_tile,
 * tile_first, tile_step; the other fields are not read) on ds's device.  It
 * holds no reference to ds.  RT_E_ARG on an empty or bad selection. */
typedef struct rt_accum rt_accum;
int rt_accum_create(const rt_dscene* ds, const rt_params* shape, rt_accum** out);
int rt_accum_free(rt_accum* acc);
/* raytracing.clj:141-155, the loop's start: enqueue sums = 0 on hip_stream;
 * the count is 0 from the call on. */
int rt_accum_clear(rt_accum* acc, void* hip_stream);
/* raytracing.clj:141-155, the loop's counter: samples per pixel of the passes
 * enqueued (and sums added) so far. */
int64_t rt_accum_samples(const rt_accum* acc);
/* One pass of the loop (raytracing.clj:141-155).  Asynchronous: trace p->spp
 * samples per pixel with the indices p->sample_begin ..., exactly as
 * rt_launch would (seed, camera, flags, depth and sample_begin are the
 * caller's: passes of one frame use consecutive sample ranges), and add their
 * integer sums to acc instead of writing a mean; the count grows by p->spp
 * at the call.  The adds are atomic: passes on several streams into one
 * accumulator are legal and give the same sums.  The adaptive tile order,
 * the sample split, RT_FLAG_STREAMED, interleaved shards, RT_FLAG_REALM and
 * RT_FLAG_REJECTION_SAMPLERS apply as to rt_launch; so does the per-launch
 * choice of the compact image (rt_set_variant: 22 / 26 where spp < 65536),
 * which looks at the pass's spp, not at the accumulated count -- a long
 * render in passes below 65536 spp stays on 22 / 26 (intended).  d_counters
 * as rt_launch.  RT_E_ARG when p's width, height or row selection differ from
 * the accumulator's, when ds is on another device, or when the count would
 * pass 2^32 - 1 (the sample index is a uint32, and one sample adds less than
 * 2^32 to a sum: the u64 cannot overflow before that); acc is unchanged then. */
int rt_launch_accum(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_accum* acc,
                    uint64_t* d_counters, void* hip_stream);
/* compute-pixel's accum / spp (raytracing.clj:141-155, :155).  Asynchronous:
 * d_out (device, rt_rows_out x width x 3 floats) = per channel
 * tot = RN(float(sum)) * 2^-24, then tot / RN(float(n)), or
 * tot * (1 / RN(float(n))) with RT_FLAG_REALM in flags (the only flag read;
 * rt_launch's other flags are accepted), n = max(count, 1) at the call.
 * This is rt_launch's own conversion: for n <= RT_MAX_SPP the frame equals
 * one launch of n spp bit for bit.  The sums are not touched: show the frame
 * and go on adding passes.  Passes enqueued on other streams must have
 * finished (or be ordered before hip_stream by the caller). */
int rt_accum_resolve(const rt_accum* acc, int flags, float* d_out, void* hip_stream);
/* The same, quantised in the same kernel (raytracing.clj:141-155, :19-26):
 * d_out (device bytes) holds what rt_quantize gives for rt_accum_resolve's
 * floats, by rt_quantize_device's threshold table. */
int rt_accum_resolve_u8(const rt_accum* acc, int flags, uint8_t* d_out, void* hip_stream);
/* The raw sums (raytracing.clj:141-155's accum, before the division) copied
 * to host_sums (rt_rows_out x width x 3 u64) behind hip_stream's work; returns
 * when they are there.  Ranks that rendered sample stripes exchange these
 * (an int64 all-reduce) and resolve once: exact weak scaling. */
int rt_accum_read(const rt_accum* acc, uint64_t* host_sums, void* hip_stream);
/* The inverse (raytracing.clj:141-155): add host_sums (the same layout) and
 * `samples` per pixel to acc, on hip_stream, atomically as a pass does;
 * returns when they are added.  RT_E_ARG when the count would pass 2^32 - 1. */
int rt_accum_add(rt_accum* acc, const uint64_t* host_sums, int64_t samples, void* hip_stream);
/* rt_accum_resolve's conversion on the host, in plain C++ (no device;
 * raytracing.clj:141-155, :155): out[i] for n sums holding `samples` per
 * pixel (0 .. 2^32 - 1), flags as rt_accum_resolve. */
int rt_resolve_sums(const uint64_t* sums, size_t n, int64_t samples, int flags, float* out);

/* ---- adaptive sampling: stop tracing tiles whose two sample halves agree ----
 * compute-pixel's loop (raytracing.clj:141-155) run only where it still
 * changes the picture.  An rt_adapt keeps two accumulators' sums, H0 and H1
 * (each rt_rows_out(shape) x width x 3 u64), one uint32 sample count per
 * 8 x 8 tile of the output rows (gy x gx of them, gx = ceil(width / 8),
 * gy = ceil(rt_rows_out / 8), row-major) and a device list of the tiles still
 * active.  Step k = 0, 1, 2, ... traces step_spp samples per pixel, with the
 * indices sample_begin + k * step_spp ..., in the active tiles only and adds
 * them to H[k & 1].  After every odd step both halves of an active tile hold
 * the same number of samples; once the tile's count has reached min_spp it is
 * tested: over its pixels inside the frame and their three channels,
 *   D = sum |H0 - H1|,  S = sum (H0 + H1),  converged iff D * 2^16 <= tol_q16 * S
 * in unbounded integers.  A converged tile leaves the active set for good, and
 * so does a tile that reaches max_spp: every active tile has the same count.
 * The sums are exact integers in any order, so the counts and the frame are a
 * function of scene, camera, seed, flags and options alone -- not of the
 * kernel variant, the sample split, the stream or the device -- and every
 * tile of the frame equals, bit for bit, the same tile of one rt_launch at
 * spp = that tile's count.
 *
 * Two properties of the rule.  Stopping on the samples' own agreement biases
 * the estimate slightly, as every half-buffer scheme does: a tile is the more
 * likely to stop the closer its two halves happen to fall, and those samples
 * are the ones kept.  And the measure is a relative L1 difference, |H0 - H1|
 * against H0 + H1: a dim but noisy tile does not meet it and runs to max_spp.
 *
 * Options: step_spp >= 1; min_spp and max_spp positive multiples of
 * 2 * step_spp with min_spp <= max_spp <= RT_MAX_SPP (sums stay below 2^56, a
 * tile's 192-term S below 2^64); tol_q16 <= 65536, the tolerance in 2^-16
 * units: 0 stops only tiles whose halves are identical, 65536 stops every
 * tile at min_spp (|a - b| <= a + b). */
typedef struct rt_adapt_opts {
  int step_spp, min_spp, max_spp;
  uint32_t tol_q16;
} rt_adapt_opts;
typedef struct rt_adapt rt_adapt;
/* raytracing.clj:141-155: an adaptive frame for `shape` (read as by
 * rt_accum_create) on ds's device: sums and counts zero, every tile active.
 * It holds no reference to ds.  RT_E_ARG on a violated option rule, an empty
 * or bad selection, or a frame of more than 65535 rows. */
int rt_adapt_create(const rt_dscene* ds, const rt_params* shape, const rt_adapt_opts* opts, rt_adapt** out);
int rt_adapt_free(rt_adapt* ad);
/* raytracing.clj:141-155, the loop's start: back to step 0, sums and counts
 * zero (enqueued on hip_stream), every tile active. */
int rt_adapt_clear(rt_adapt* ad, void* hip_stream);
/* One step of the loop (raytracing.clj:141-155).  Enqueues the trace of
 * step_spp samples per pixel over the active tiles -- rt_launch_accum's pass
 * with the active list as its tile order: the trace kernel is the same on
 * every variant -- and behind it, after an odd step, the rule's kernel.
 * p->spp is ignored; p->sample_begin is the frame's first index, the same at
 * every step (the step's offset is the library's).  Seed, camera, depth,
 * RT_FLAG_REALM, RT_FLAG_REJECTION_SAMPLERS, RT_FLAG_STREAMED and the sample
 * split apply as to rt_launch_accum, the split computed from the number of
 * active tiles, so that a thin late step still fills the device.  The steps
 * neither read nor write the stream's tile-cost record (rt_set_schedule).
 * Returns the number of tiles traced; 0 when no tile is active: nothing is
 * enqueued then and d_counters is left alone.  The grid of a launch depends
 * on the active count, so the step after a tested one first waits for that
 * test and reads its two numbers back through pinned memory (8 bytes): one
 * host sync every two steps.  The steps of a frame go on one stream (or are
 * ordered by the caller).  RT_E_ARG when p's width, height or row selection
 * differ from the frame's, when ds is on another device, or when the launch's
 * kernel variant has no 8 x 8 tiles (rt_set_variant 28, the diagnostic
 * 20 / 21); the frame is unchanged then. */
int rt_adapt_step(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_adapt* ad,
                  uint64_t* d_counters, void* hip_stream);
/* raytracing.clj:141-155: the tiles still active, as of the last test read
 * back (no wait). */
int rt_adapt_active(const rt_adapt* ad);
/* raytracing.clj:141-155, the loop's counter: samples traced so far, summed
 * over the frame's pixels. */
int64_t rt_adapt_samples(const rt_adapt* ad);
/* compute-pixel's accum / spp with each tile's own count
 * (raytracing.clj:141-155, :155).  Asynchronous, non-destructive: d_out
 * (device, rt_rows_out x width x 3 floats) = per channel
 * RN(float(H0 + H1)) * 2^-24 / RN(float(count[tile])), or * (1 / RN(float(
 * count))) with RT_FLAG_REALM in flags (the only flag read) -- rt_launch's own
 * conversion; a count of 0 divides by 1. */
int rt_adapt_resolve(const rt_adapt* ad, int flags, float* d_out, void* hip_stream);
/* The same, quantised in the same kernel by rt_quantize_device's threshold
 * table (raytracing.clj:141-155, :19-26): the bytes rt_quantize gives for
 * rt_adapt_resolve's floats. */
int rt_adapt_resolve_u8(const rt_adapt* ad, int flags, uint8_t* d_out, void* hip_stream);
/* One half of the frame as a frame of its own (raytracing.clj:141-155, :155),
 * so that an adaptive frame's two estimates feed rt_denoise without a trip
 * through the host.  Asynchronous, non-destructive: d_out (device,
 * rt_rows_out x width x 3 floats) = per channel RN(float(H[half])) * 2^-24 /
 * RN(float(max(count[tile] / 2, 1))), or * (1 / that) with RT_FLAG_REALM in
 * flags (the only flag read) -- what rt_adapt_resolve_host gives for
 * (H[half], zeros, counts / 2).  After an even number of steps each half
 * holds count / 2 samples.  RT_E_ARG for a half outside {0, 1}. */
int rt_adapt_resolve_half(const rt_adapt* ad, int half, int flags, float* d_out, void* hip_stream);
/* raytracing.clj:141-155: the gy x gx samples per pixel of the tiles, the
 * frame's sample heat map, copied to host_counts behind hip_stream's work;
 * returns when they are there. */
int rt_adapt_counts(const rt_adapt* ad, uint32_t* host_counts, void* hip_stream);
/* raytracing.clj:141-155's accum, both halves (rt_accum_read's layout each):
 * the sums of the even steps into host_sums0, of the odd steps into
 * host_sums1; returns when they are there. */
int rt_adapt_read(const rt_adapt* ad, uint64_t* host_sums0, uint64_t* host_sums1, void* hip_stream);
/* The rule on the host, in plain C++ (no device; raytracing.clj:141-155):
 * converged[ty * gx + tx] = 1 where tile (tx, ty) of the rows x width frame
 * whose halves are sums0 and sums1 meets D * 2^16 <= tol_q16 * S, else 0. */
int rt_adapt_eval_host(const uint64_t* sums0, const uint64_t* sums1, int width, int rows, uint32_t tol_q16,
                       uint8_t* converged);
/* rt_adapt_resolve's conversion on the host, in plain C++ (no device;
 * raytracing.clj:141-155, :155): out (rows x width x 3) from the two halves
 * and the gy x gx counts, flags as rt_adapt_resolve. */
int rt_adapt_resolve_host(const uint64_t* sums0, const uint64_t* sums1, const uint32_t* counts, int width,
                          int rows, int flags, float* out);

/* ---- first-hit features: albedo, normal, depth and coverage -----------------
 * Noise-free per-pixel guides for a denoiser or a compositor: what the first
 * surface a camera ray meets looks like.  For pixel (i, j) and sample index k
 * a feature launch traces exactly the camera ray rt_launch traces for that
 * (seed, pixel, sample) -- the same RNG stream, jitter, defocus draw (loop-free
 * or by rejection, RT_FLAG_REJECTION_SAMPLERS) and d = s - o
 * (raytracing.clj:144-151) -- runs one hit-anything on it (raytracing.clj:33-43,
 * the kernel's fp32 body test and first-wins tie rule) and adds the result to
 * integer sums, so that passes, shards and streams combine exactly, in any
 * order, as they do for an rt_accum.  Per sample:
 *   hit:  albedo = the body's ::attenuation (material.clj:13-46): its rgb for
 *         RT_LAMBERTIAN and RT_METAL, (1, 1, 1) for RT_DIELECTRIC (:46),
 *         (0, 0, 0) for RT_NONE; normal = the hit record's face-corrected unit
 *         normal (hittable.clj:24-31, hit.clj:14-15: (P - C) / r, turned
 *         against the ray, then scaled by 1 / its own length: the fp32 root
 *         leaves P off the surface, and (P - C) / r up to 1e-3 off unit
 *         length for a small distant body); t = the Euclidean distance from
 *         the ray's origin
 *         (the reference's ::hit/t times |d|);
 *   miss: albedo = the sky colour of that ray (raytracing.clj:55-58), normal 0,
 *         no distance, not counted as a hit.
 * Kept per pixel: six 64-bit sums in 2^-24 units (albedo rgb, each sample
 * clamped as a colour is, RT_MAX_SPP; normal xyz, signed, toward zero), a
 * uint32 count of hit samples, and the MINIMUM of t over the hit samples
 * (+inf: none) -- the nearest surface in the pixel, not a mean distance: a
 * minimum is exact in any order at every scene scale.  The resolved normal is
 * the mean over all samples with misses as zero and is NOT re-normalised: its
 * length falls below 1 where a pixel sees several surfaces or the sky.
 * RT_FLAG_REALM is accepted and changes nothing (both namespaces share the
 * camera and the sphere), RT_FLAG_STREAMED likewise; max_depth is not read.
 *
 * rt_feat_create (raytracing.clj:141-155, the loop's state): empty feature
 * buffers for frames of `shape` (read and checked as rt_accum_create does) on
 * ds's device, cleared (depth +inf).  It holds no reference to ds. */
#define RT_FEAT_CHANNELS 8
typedef struct rt_feat rt_feat;
int rt_feat_create(const rt_dscene* ds, const rt_params* shape, rt_feat** out);
int rt_feat_free(rt_feat* f);
/* raytracing.clj:141-155, the loop's start: enqueue sums = 0, hits = 0,
 * depth = +inf on hip_stream; the count is 0 from the call on. */
int rt_feat_clear(rt_feat* f, void* hip_stream);
/* raytracing.clj:141-155, the loop's counter: samples per pixel of the passes
 * enqueued so far. */
int64_t rt_feat_samples(const rt_feat* f);
/* One pass (raytracing.clj:144-151, :33-43, hittable.clj:7-31,
 * material.clj:13-46).  Asynchronous: trace the first segment of p->spp
 * samples per pixel, indices p->sample_begin ..., and add them to f by
 * atomics: passes from several streams into one rt_feat are legal and give the
 * same contents.  Interleaved row selections as rt_launch_accum.  d_counters:
 * NULL or device u64[2] += {samples traced, samples traced} (one segment per
 * sample).  rt_set_variant chooses where the kernel reads the bodies (5: the
 * linear scan; 12: the BVH in global memory; otherwise the BVH in LDS where it
 * fits): the contents never depend on it.  The stream's tile-cost record
 * (rt_set_schedule) is neither read nor written.  RT_E_ARG when p's width,
 * height or row selection differ from f's, when ds is on another device, when
 * the count would pass 2^32 - 1, or when f holds specular-chain passes
 * (rt_launch_feat_chain, below); f is unchanged then. */
int rt_launch_feat(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_feat* f,
                   uint64_t* d_counters, void* hip_stream);
/* compute-pixel's accum / spp for the features (raytracing.clj:155).
 * Asynchronous, non-destructive: d_out (device, rt_rows_out x width x
 * RT_FEAT_CHANNELS floats) = per pixel, with nf = RN(float(max(count, 1))):
 *   [0..2] albedo rgb  RN(float(sum)) * 2^-24 / nf  (rt_launch's conversion)
 *   [3..5] normal xyz  the same from the signed sums
 *   [6]    depth       the minimum, or +inf
 *   [7]    coverage    RN(float(hits)) / nf */
int rt_feat_resolve(const rt_feat* f, float* d_out, void* hip_stream);
/* raytracing.clj:141-155's accum, raw: host_sums (rt_rows_out x width x 6
 * int64: albedo rgb, normal xyz), host_hits and host_depth (rt_rows_out x
 * width each) copied behind hip_stream's work; returns when they are there. */
int rt_feat_read(const rt_feat* f, int64_t* host_sums, uint32_t* host_hits, float* host_depth, void* hip_stream);
/* The inverse (raytracing.clj:141-155): merge rt_feat_read's arrays of another
 * rt_feat of the same shape (a rank's sample stripe) and its `samples` per
 * pixel into f, on hip_stream, atomically as a pass does -- sums and hit
 * counts added, the depth by minimum; returns when they are merged.  RT_E_ARG
 * when the count would pass 2^32 - 1 or a depth is not a positive distance
 * or +inf; f is unchanged then. */
int rt_feat_add(rt_feat* f, const int64_t* host_sums, const uint32_t* host_hits, const float* host_depth,
                int64_t samples, void* hip_stream);
/* rt_feat_resolve's conversion on the host, in plain C++ (no device;
 * raytracing.clj:155): out (n_px x RT_FEAT_CHANNELS) from rt_feat_read's
 * arrays holding `samples` per pixel (0 .. 2^32 - 1).  The albedo sums are
 * read as unsigned. */
int rt_feat_resolve_host(const int64_t* sums, const uint32_t* hits, const float* depth, size_t n_px,
                         int64_t samples, float* out);
/* The feature kernel a launch on ds would run under the current selector
 * (diagnostic; raytracing.clj:33-43's scan as it is run): out4 = {workgroups
 * per CU, VGPRs per lane, LDS bytes per workgroup, the bodies' source: 0 = BVH
 * in LDS, 1 = BVH in global memory, 2 = linear scan}. */
int rt_feat_occupancy(const rt_dscene* ds, int* out4);

/* ---- specular-chain features: guides for what glass and mirrors show ------------
 * rt_launch_feat stops at the first surface: on a mirror or on glass every
 * pixel then has one albedo and a smooth normal and depth, and a denoiser or an
 * upsampler guided by them treats the reflected or refracted scene as paint on
 * that surface.  A chain pass follows the deterministic part of ray-color's
 * recursion (raytracing.clj:45-58) from the same camera ray to the first rough
 * surface, or to the sky, and takes the features there.  It adds to an rt_feat
 * in rt_launch_feat's units, so rt_feat_resolve, _read, _add, _resolve_host,
 * rt_denoise and rt_upsample take its result as they take the first-hit one.
 *
 * Per sample, in fp32, every fma written out (the trace kernel's operations;
 * sqrt and 1/x correctly rounded): the ray (o, d) is rt_launch_feat's camera
 * ray; thr = (1, 1, 1), L = 0, last = -1 (no body), b = 0.  Then, repeated:
 *   1. u = d * (1 / |d|), t-min = 1e-3 in |d| units (raytracing.clj:48).
 *   2. The closest hit as rt_launch_ids' step 2 finds it, with the trace
 *      kernel's self-hit guard: for the body `last` the root is taken with |h|
 *      in place of sqrt(disc) (the origin lies on that body: exact arithmetic
 *      has cc = 0).  With last = -1 this is rt_launch_feat's search bit for bit.
 *   3. No hit: albedo_c = thr_c * sky_c (raytracing.clj:55-58, from u), normal
 *      0, not a hit, no depth.  The chain ends.
 *   4. A hit at t: L = L + t.  P = o + t u, n = (P - C) * (1 / r), turned
 *      against d (hittable.clj:24-31, hit.clj:14-15).  The body is smooth iff it
 *      is RT_DIELECTRIC, or RT_METAL with fuzz <= fuzz_max (a NaN fuzz is not).
 *   5. Smooth, and b < max_bounces:
 *      metal (material.clj:21-28 with the fuzz term dropped: no random vector
 *        is drawn; at fuzz 0 this is the reference's direction exactly):
 *        rdir = d - 2 dot(d, n) n on the un-normalised d.  Unless
 *        dot(rdir, n) > 0 the chain ends here as in 6; else thr_c *= albedo_c,
 *        d = rdir.
 *      dielectric (realm/raytracing.clj:158-177, the branch RT_FLAG_REALM runs:
 *        no Schlick term, no draw): ri = 1 / index on a front face, the index on
 *        a back face; cos = min(-dot(u, n), 1), sin = sqrt(1 - cos^2); total
 *        internal reflection of u iff not (ri * sin <= 1), else vec3a.clj:97-101's
 *        refraction.  thr is unchanged.
 *      Then o = P, last = the body, b = b + 1, and back to 1.
 *   6. Otherwise the chain ends on this surface: albedo_c = thr_c * att_c with
 *      rt_launch_feat's ::attenuation (the body's rgb, 1 for glass, 0 for
 *      RT_NONE), the normal n scaled by one correctly rounded 1 / |n|, a hit,
 *      depth = L.
 * Accumulated as rt_launch_feat accumulates: the six sums, the hit count, the
 * minimum of L over the hit samples.
 *
 * Two properties (tests/test_chain_host.py, tests/test_gpu_chain.py):
 *  - with max_bounces = 0, or on a scene without smooth bodies, every sample is
 *    rt_launch_feat's bit for bit (1 * x, 0 + t and the unguarded test are exact);
 *  - on a scene of smooth bodies only the chain is the path rt_launch traces
 *    under RT_FLAG_REALM: the same segments, the same bits.
 *
 * What a user must know:
 *  - Depth is a VIRTUAL distance: camera to the rough surface along the bends,
 *    the minimum over the pixel's hit samples.  It is no distance from the
 *    camera to anything, and a reprojection through it is wrong: chain features
 *    must never be given to rt_temporal_step* or rt_temporal_probe.  A sequence
 *    keeps a first-hit rt_feat for those and a chain rt_feat for rt_denoise and
 *    rt_upsample.
 *  - The normal is the last surface's in world space.  It is not mirrored into
 *    the reflecting surface's frame.
 *  - Glass takes the refraction branch only, as under RT_FLAG_REALM.  The glass's
 *    own faint reflection, which the default namespace draws by Schlick's
 *    reflectance (material.clj:30-46), is not followed: the guides describe what
 *    is seen through the glass, and the reflection on it is filtered as before.
 *  - Metal with fuzz above fuzz_max is rough: the chain ends on it with its own
 *    albedo.  Metal at or below it is followed as a perfect mirror.
 *  - Coverage is the share of samples whose chain ended on a surface.
 *  - A chain that runs out of bounces ends on the smooth surface it is on.
 *
 * NULL options: {8, 0.0f}.  max_bounces 0 .. 64, fuzz_max finite and >= 0, else
 * RT_E_ARG. */
typedef struct rt_feat_chain_opts {
  int max_bounces;   /* smooth surfaces passed per sample, at most             */
  float fuzz_max;    /* metal with fuzz <= this is followed as a mirror        */
} rt_feat_chain_opts;
/* One chain pass (raytracing.clj:45-58, :33-43, :144-151, hittable.clj:7-31,
 * material.clj:13-46, realm/raytracing.clj:158-177) added to f exactly as
 * rt_launch_feat adds one: the same checks, row selections, samplers, streams
 * and selector; RT_FLAG_REALM and RT_FLAG_STREAMED are accepted and inert.
 * d_counters: NULL or device u64[2] += {segments traced, samples traced}.
 * An rt_feat remembers which kind of pass it holds since its last clear: a
 * chain pass into one that holds first-hit passes, rt_launch_feat into one that
 * holds chain passes, or a chain pass with other options than the ones it
 * holds, is RT_E_ARG with f unchanged.  rt_feat_clear lifts the kind,
 * rt_feat_add keeps it.  All argument errors are returned before anything is
 * enqueued. */
int rt_launch_feat_chain(const rt_dscene* ds, const rt_camera* c, const rt_params* p, const rt_feat_chain_opts* opts,
                         rt_feat* f, uint64_t* d_counters, void* hip_stream);
/* The chain of one ray on the host, in plain C++ (no device; the same text the
 * kernel runs, over raytracing.clj:33-43's scan in array order): rays = n x
 * (o, d) float32, e.g. a camera's samples; out[i] = the body the chain ended on
 * (-1: the sky), the bounces taken, L (+inf on the sky), and the albedo and
 * normal floats before their conversion to 2^-24 units.  The yardstick of the
 * kernel.  RT_E_MATERIAL on an unknown material kind. */
typedef struct rt_chain_sample {
  int32_t body, bounces;
  float length, albedo[3], normal[3];
} rt_chain_sample;
int rt_feat_chain_host(const rt_scene* s, const rt_feat_chain_opts* opts, const float* rays, size_t n,
                       rt_chain_sample* out);
/* The chain kernel a launch on ds would run under the current selector
 * (diagnostic; raytracing.clj:33-43's scan as it is run): out4 as
 * rt_feat_occupancy's. */
int rt_feat_chain_occupancy(const rt_dscene* ds, int* out4);

/* ---- body ids: which body a pixel shows -----------------------------------------
 * The index hit-anything's reduce (raytracing.clj:33-43) ends on, per pixel,
 * for the pixel centre's pinhole ray: an object-id buffer (picking, masks), and
 * what rt_temporal_step_motion needs to know whose displacement to subtract.
 * The device kernel and rt_ids_host give the same integers.
 *
 * Image: rows x width int32, contiguous; image row y is camera row row0 + y (a
 * contiguous row band, as rt_temporal_create's).
 * Per pixel (x, y), j = row0 + y:
 *   1. The ray is the one rt_temporal_step's step 1 uses: origin = center,
 *      direction e_c = ((p00_c + float(x) * du_c) + float(j) * dv_c) - center_c,
 *      each operation one fp32 operation rounded once (no fma); no jitter, no
 *      defocus, no random number.
 *   2. The closest hit of (center, e) over the bodies as rt_launch_feat finds
 *      it: |e| and 1 / |e| correctly rounded, u = e * (1 / |e|), t-min = 1e-3 in
 *      |e| units; per body (centre c, radius r), with oc = c - center, in fp32
 *      with the fma written out: h = fma(u_z, oc_z, fma(u_y, oc_y, u_x * oc_x)),
 *      cc = fma(oc_x, oc_x, fma(oc_z, oc_z, fma(oc_y, oc_y, -(r * r)))),
 *      disc = fma(h, h, -cc); no root unless min(disc, max(h, -cc)) >= 0; the
 *      root t = h - sqrt(disc) if that is > t-min, else h + sqrt(disc); accepted
 *      iff t > t-min and (t, index) is lexicographically below the best so far
 *      (ties go to the lower index; no self-hit guard: a camera ray leaves no
 *      body).  A body whose radius is NaN or infinite, or whose r * r overflows,
 *      is never hit.
 *   3. ids[y * width + x] = the body's index in the scene's array order, or -1
 *      where nothing is hit.
 * The device reads the tree rt_scene_upload made (or scans, as rt_launch_feat
 * does under rt_set_variant: 5 the scan, 12 the tree in global memory,
 * otherwise the tree in LDS where it fits -- the faster of the two trees even
 * at one ray a thread); the walk gives the scan's answer bit
 * for bit.
 *
 * To know: the id is the pinhole centre's body, while rt_feat's depth is the
 * nearest hit over jittered, defocused rays -- on a silhouette pixel the two
 * can belong to different bodies. */
/* raytracing.clj:33-43's index, on the device.  Asynchronous, on hip_stream
 * (NULL: the default stream) of ds's device: d_ids (device, rows x width
 * int32) is written, every element.  RT_E_ARG on a NULL argument, width or
 * rows <= 0, more than 2^31 - 1 pixels, a negative row0, or a stream of another
 * device -- before anything is enqueued. */
int rt_launch_ids(const rt_dscene* ds, const rt_camera* c, int width, int rows, int row0, int32_t* d_ids,
                  void* hip_stream);
/* The same on the host, in plain C++ (no device; raytracing.clj:33-43's scan in
 * array order, over the (centre, -r^2) table rt_scene_upload builds): the
 * yardstick of the kernel, and ids for frames that are on the host. */
int rt_ids_host(const rt_scene* s, const rt_camera* c, int width, int rows, int row0, int32_t* out);
/* The body-id kernel a launch on ds would run under the current selector
 * (diagnostic; raytracing.clj:33-43's scan as it is run): out4 as
 * rt_feat_occupancy's. */
int rt_ids_occupancy(const rt_dscene* ds, int* out4);
/* How far each body of raytracing.clj:63-78's scene moved between two frames:
 * out (n x 4 floats) = per body b, out[4 b + c] = cur.center_c - prev.center_c
 * (one fp32 subtraction per component, c = 0, 1, 2) and out[4 b + 3] = 0.  A
 * body whose radius, material kind or any of its four material floats differs
 * by bits between the scenes has no past: its three components are NaN (which
 * rt_temporal_step_motion turns into "no history").  RT_E_ARG on a NULL
 * argument or when the body counts differ.  Only rigid translation is
 * described; a sphere's rotation is invisible with one albedo per body. */
int rt_body_motion(const rt_scene* cur, const rt_scene* prev, float* out);

/* ---- ray queries: closest hit and occlusion for the caller's rays ---------------
 * hit-anything (raytracing.clj:33-43) over the sphere ::hit-fn
 * (hittable.clj:7-31) for rays the caller brings: a pick through the real lens,
 * line of sight between two bodies, a collision probe, a shadow or occlusion
 * test -- answered by the search the renderer itself runs, on the tree
 * rt_scene_upload built and rt_scene_update refits.  The device kernels and
 * the host entries give the same bits.
 *
 * Per ray i (o, t_min, d, t_max), in fp32 with every fma written out:
 *   1. Set-up, as rt_launch_ids' step 2: |d| = sqrt(fma(d_z, d_z, fma(d_y, d_y,
 *      d_x * d_x))) and 1 / |d| correctly rounded, u = d * (1 / |d|).  The lower
 *      bound is tmin = t_min * |d|, one multiplication (t_min = 1e-3f gives
 *      raytracing.clj:48's t-min as rt_launch_ids computes it, bit for bit); the
 *      search starts from the best (t_max * |d|, no body), and a root is accepted
 *      only if it is below the best: t_max is a strict upper bound, +inf is none.
 *   2. The ray is inactive if a component of o is not finite; if |d| as
 *      computed is 0 (d is zero, or its square underflows), infinite (also where
 *      the square overflows) or NaN; if t_min is NaN or negative; if t_max is
 *      NaN or t_max <= t_min; or if the two products leave no interval
 *      (t_min * |d| < t_max * |d| fails).  An inactive ray is not searched: its
 *      record is the "none" record {-1, 0, +inf, +inf, 0, 0, 0, 0}, its
 *      occlusion byte 0.
 *   3. The closest hit is rt_launch_ids' step 2 with these bounds: the same body
 *      test, ties to the lower index.  With last[i] >= 0 the body last[i] takes
 *      the trace kernel's self-hit guard (|h| in place of sqrt(disc), as in
 *      rt_launch_feat_chain's step 2): for a ray that leaves that body's
 *      surface.  last == NULL or last[i] < 0: no guard; last[i] >= the body
 *      count names no body and is no error; nor does a body that can never be
 *      hit (a centre or radius that is NaN or infinite, an r * r that overflows):
 *      the guard needs no disc, so on such a body it would invent a root.
 *   4. The record of a hit on body b at the accepted root `dist`:
 *      t = dist * (1 / |d|), one multiplication.  The normal is hittable.clj:
 *      24-31's (P - C) * (1 / r), with P - C rebuilt around the ray's closest
 *      point to the centre rather than from P = o + dist * u: with oc = C - o
 *      and h as in step 3, w_c = fma(-h, u_c, oc_c), b2 = fma(w_z, w_z,
 *      fma(w_y, w_y, w_x * w_x)), s = sqrt(max(r * r - b2, 0)) correctly
 *      rounded (r * r the product step 3 uses), taken with + if dist > h (the
 *      farther root, the guard's too) and with - otherwise, and
 *      n_c = fma(+-s, u_c, -w_c) * (1 / r).  Then hit.clj:14-15 as
 *      rt_launch_feat reads it: front_face = dot(d, n) < 0 on the un-normalised
 *      d, n turned against d and scaled by one correctly rounded 1 / |n|.  A
 *      component that comes out NaN (a body of radius 0 hit in its centre) is
 *      stored as 0, as rt_feat's sums take it.  A ray that meets nothing has
 *      the "none" record.
 *   5. occluded[i] = 1 iff step 3 finds a body, else 0.  The occlusion kernel
 *      stops at the first body the test accepts against (tmin, t_max * |d|).
 * The device follows rt_set_variant as rt_launch_ids does (5: the scan, 12: the
 * tree in global memory, else the tree in LDS where it fits); the walk gives
 * the scan's answer bit for bit (tests/test_rays_host.py holds that on query
 * rays: origins far outside and deep inside bodies, t_min = 0, finite t_max,
 * |d| from 2^-6 to 2^6).
 *
 * To know: dist lies within about 6e-4 * (|C - o| + r) of the exact root (the
 * fp32 test's position error: it is the depth rt_launch_feat records, bit for
 * bit, for the same ray).  The normal does not inherit that error: the
 * discriminant's cancellation at the size of |C - o|^2 would put it off by
 * 8e-3 a component on a body of r = 0.2 met 27 units away, while s comes from
 * numbers of the size of r -- within 1e-4 of the exact normal there
 * (tests/test_rays_host.py).  On such a hit it is more exact than the normal
 * rt_launch_feat accumulates, and differs from it. */
typedef struct rt_ray {      /* 32 bytes, 16-byte aligned on the device */
  float o[3];  float t_min;  /* origin; lower bound of the ray parameter, in units of |d| */
  float d[3];  float t_max;  /* direction, any length; upper bound, +inf = unbounded      */
} rt_ray;
typedef struct rt_ray_hit {  /* 32 bytes, 16-byte aligned on the device */
  int32_t body;              /* index in the scene's array order, -1: none                */
  int32_t front_face;        /* hit.clj:14-15: dot(d, outward normal) < 0; 0 when none    */
  float t;                   /* ray parameter in units of |d|: dist * RN(1/|d|)           */
  float dist;                /* the distance the search found (rt_feat's depth unit)      */
  float normal[3];           /* (P - C) * (1/r), turned against d (hittable.clj:24-31)    */
  float reserved;            /* 0 */
} rt_ray_hit;
/* raytracing.clj:33-43 and hittable.clj:7-31 for n caller-supplied rays, on the
 * device.  Asynchronous, on hip_stream (NULL: the default stream) of ds's
 * device: d_hits[0 .. n) is written, every word.  d_rays, d_hits: device
 * memory, 16-byte aligned; d_last: NULL or n int32 on the device.  RT_E_ARG on
 * a NULL argument other than d_last (the arrays may be NULL when n == 0), a
 * misaligned d_rays or d_hits, n > 2^31 - 1, or a stream of another device --
 * before anything is enqueued.  n == 0 is RT_OK and enqueues nothing. */
int rt_launch_rays(const rt_dscene* ds, const rt_ray* d_rays, const int32_t* d_last, size_t n, rt_ray_hit* d_hits,
                   void* hip_stream);
/* raytracing.clj:33-43's "some body" for the same rays: d_occluded[0 .. n) is
 * written, one byte a ray (step 5).  Arguments and errors as rt_launch_rays'
 * (d_occluded needs no alignment). */
int rt_launch_occluded(const rt_dscene* ds, const rt_ray* d_rays, const int32_t* d_last, size_t n, uint8_t* d_occluded,
                       void* hip_stream);
/* The same on the host, in plain C++ (no device; raytracing.clj:33-43's scan in
 * array order with hittable.clj:7-31's test, the text the kernels run): the
 * yardstick of the kernels, and queries against scenes that are on the host.
 * last: NULL or n int32.  RT_E_ARG on a NULL argument other than last (with
 * n > 0) or n > 2^31 - 1. */
int rt_rays_host(const rt_scene* s, const rt_ray* rays, const int32_t* last, size_t n, rt_ray_hit* out);
int rt_occluded_host(const rt_scene* s, const rt_ray* rays, const int32_t* last, size_t n, uint8_t* out);
/* The closest-hit kernel a launch on ds would run under the current selector
 * (diagnostic; raytracing.clj:33-43's scan as it is run): out4 as
 * rt_ids_occupancy's. */
int rt_rays_occupancy(const rt_dscene* ds, int* out4);

/* ---- feature-guided denoiser: an a-trous filter over rt_feat's guides --------
 * What a low-sample frame of compute-pixel's loop (raytracing.clj:141-155)
 * looks like after an edge-avoiding a-trous wavelet filter (Dammertz et al.
 * 2010) guided by rt_feat_resolve's eight channels, run on albedo-demodulated
 * colour, its colour edge-stop scaled by the variance two half-frames give (the
 * SVGF manner).  The result is a function of the inputs and options alone: a
 * fixed sequence of single fp32 operations, each rounded once in the order
 * written (no fma; / and sqrt IEEE), which the device kernels, rt_denoise_host
 * and a NumPy restatement (tests/test_denoise_host.py) give bit for bit,
 * whatever the workgroup shape.
 *
 * Inputs, for a contiguous rows x width image (neighbours in the arrays must
 * be neighbours in the picture: a compacted interleaved shard, tile_step > 0,
 * is gathered first):
 *   half0, half1  rows x width x 3 floats each: two estimates of the frame from
 *                 disjoint, equally large sample sets (two rt_accum over sample
 *                 ranges [0, n) and [n, 2 n); rt_adapt_resolve_half's two);
 *   feat          rows x width x 8 floats in rt_feat_resolve's layout: albedo
 *                 rgb, normal xyz, depth (+inf where nothing was hit), coverage.
 * Options (NULL: the defaults; outside the ranges: RT_E_ARG):
 *   levels       5     1..8      a-trous levels, step 2^i at level i
 *   normal_pow2  5     0..8      the normal weight is squared this many times
 *   sigma_c      4.0   finite > 0  colour edge-stop, in standard deviations
 *   sigma_z      0.05  finite > 0  depth edge-stop, relative depth per pixel
 *
 * Prep, per pixel p:
 *   alb_c = max(feat_c, 2^-10), c = r, g, b
 *   ia = half0 / alb, ib = half1 / alb, m = 0.5 * (ia + ib)
 *   lum(x) = (x_r * 0.2126f + x_g * 0.7152f) + x_b * 0.0722f
 *   d = lum(ia) - lum(ib), var = (0.25f * d) * d
 *   texel (m_r, m_g, m_b, var); guides n = feat[3..5], z = feat[6],
 *   cov = feat[7], the same at every level.
 * Level i = 0 .. levels - 1, step s = 2^i, from the previous texels to new ones:
 *   1. vbar_p = the 3 x 3 binomial mean of var at step 1: weights
 *      k = g[dy] * g[dx], g = {1/4, 1/2, 1/4} (exact), taps row-major (dy outer)
 *      over -1..1, taps outside the image skipped, num += k * var_q and
 *      den += k from 0 in that order, vbar = num / den.
 *   2. sd = sqrt(vbar) * sigma_c + 1e-6f.
 *   3. Taps (dy, dx), each -2..2, row-major (dy outer), at q = p + s * (dx, dy),
 *      those outside the image skipped; k = h[dy] * h[dx],
 *      h = {1/16, 1/4, 3/8, 1/4, 1/16} (exact).  The centre tap has w = k.
 *      Every other tap:
 *        dn = min(1, max(0, ((n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z)
 *                           + (1 - cov_p) * (1 - cov_q)))
 *             (sky agrees with sky; a surface never agrees with sky)
 *        wn = dn, squared normal_pow2 times
 *        wz = 1 where z_p and z_q are both +inf, 0 where exactly one is, else
 *             r = |z_p - z_q| / ((sigma_z * float(s * max(|dx|, |dy|))) * min(z_p, z_q)),
 *             wz = 1 / (1 + r * r)
 *        rc = |lum(m_p) - lum(m_q)| / sd, wc = 1 / (1 + rc * rc)
 *        w = ((k * wn) * wz) * wc
 *      and in tap order, from 0:  acc_c += w * m_q.c,  accv += (w * w) * var_q,
 *      wsum += w.
 *   4. m' = acc / wsum, var' = accv / (wsum * wsum)  (wsum >= 9/64: the centre).
 * Output: out_c = m_c * alb_c after the last level.
 *
 * To know: the filter biases (it trades noise for blur: the more samples a
 * frame holds the less it gains); glass and mirrors are guided
 * by their first hit only, so what they show is filtered as one surface; the
 * depth term is relative depth per pixel of tap distance, not distance from a
 * plane, so ground seen at a grazing angle is filtered less.
 *
 * The inputs are never written.  out may not overlap an input (RT_E_ARG).
 * Inputs are expected as the library produces them (finite colours, features
 * as rt_feat_resolve writes them); other values -- NaN, a depth <= 0 -- give
 * unspecified numbers, never an out-of-bounds access, a fault or a hang. */
typedef struct rt_denoise_opts {
  int levels, normal_pow2;
  float sigma_c, sigma_z;
} rt_denoise_opts;
typedef struct rt_denoiser rt_denoiser;
/* raytracing.clj:141-155's frame, filtered: a denoiser for rows x width images
 * on `device`.  It owns the two ping-pong texel buffers and the packed guides
 * (16 + 16 + 16 + 4 = 52 bytes per pixel) and nothing else.
 * RT_E_ARG on width or rows <= 0 or more than 2^31 - 1 pixels, RT_E_NODEV on
 * a device that is not there. */
int rt_denoiser_create(int device, int width, int rows, rt_denoiser** out);
int rt_denoiser_free(rt_denoiser* dn);   /* NULL: 0 */
/* Asynchronous: enqueue the filter on hip_stream (NULL: the default stream) of
 * the denoiser's device: the prep, then one kernel per level, the last of
 * which writes d_out (device, rows x width x 3 floats).  d_half0, d_half1 and
 * d_feat are device pointers, aligned as floats.  Calls on one denoiser share
 * its scratch: they go on one stream, or are ordered by the caller.  RT_E_ARG
 * on a NULL argument, bad options, d_out overlapping an input, or a stream of
 * another device. */
int rt_denoise(rt_denoiser* dn, const rt_denoise_opts* o, const float* d_half0, const float* d_half1,
               const float* d_feat, float* d_out, void* hip_stream);
/* rt_denoise with a HIP event behind every kernel (diagnostic; synchronous,
 * raytracing.clj:141-155's frame as above): waits for the filter, then out_ms
 * (levels + 2 floats) = the milliseconds of the prep, of each level in order,
 * and of the whole from the first event to the last. */
int rt_denoise_profile(rt_denoiser* dn, const rt_denoise_opts* o, const float* d_half0, const float* d_half1,
                       const float* d_feat, float* d_out, void* hip_stream, float* out_ms);
/* The same on the host, in plain C++ (no device; raytracing.clj:141-155): the
 * yardstick of the kernels, and a filter for frames that are on the host. */
int rt_denoise_host(const rt_denoise_opts* o, const float* half0, const float* half1, const float* feat,
                    int width, int rows, float* out);

/* ---- guided upsampling: colour traced on a coarse grid, rebuilt at full size ----
 * A render scale: compute-pixel's loop (raytracing.clj:141-155) run for the
 * frame of rt_camera_coarsen's camera (raytracing.clj:129-135), one pixel per
 * s x s block of the frame's pixels, and its colour brought up to the frame's
 * size through the frame's own first-hit features -- a joint bilateral
 * upsampling (Kopf et al. 2007) of albedo-demodulated colour with rt_denoise's
 * normal, coverage and depth weights.  The output has rt_denoise's and
 * rt_temporal_step's input shape and feeds them unchanged.  The result is a
 * function of the inputs and options alone: a fixed sequence of single fp32
 * operations, each rounded once in the order written (no fma; / IEEE), which
 * the device kernel, rt_upsample_host and a NumPy restatement
 * (tests/test_upsample_host.py) give bit for bit, whatever the workgroup shape.
 *
 * Inputs, for a full-size image of rows x width pixels and s = scale, with
 * cw = ceil(width / s), ch = ceil(rows / s):
 *   half0, half1  ch x cw x 3 floats each: two estimates of the coarse frame
 *                 from disjoint sample sets (half1 and out1 may both be NULL:
 *                 one image; exactly one of them NULL is RT_E_ARG);
 *   feat_coarse   ch x cw x 8 floats in rt_feat_resolve's layout, the coarse
 *                 camera's features;
 *   feat          rows x width x 8 floats likewise, the frame's own features.
 * Outputs: out0, out1, rows x width x 3 floats each.
 * Options (NULL: the defaults; outside the ranges: RT_E_ARG):
 *   scale        2     2..4
 *   normal_pow2  0     0..8        the normal weight is squared this many times
 *   sigma_z      0.05  finite > 0  depth edge-stop, relative depth per fine pixel
 *
 * Per fine pixel p = (x, y):
 *   1. Along x: ux = 2 x + 1 - s, X0 = floor(ux / 2 s) (an integer; -1 in the
 *      first columns), ax = ux - 2 s X0 in [0, 2 s),
 *      bx0 = float(2 s - ax) / float(2 s), bx1 = float(ax) / float(2 s).
 *      The same along y.
 *   2. Taps (Y0, X0), (Y0, X0 + 1), (Y0 + 1, X0), (Y0 + 1, X0 + 1) in that
 *      order, those outside the coarse image skipped; b = by * bx.
 *   3. Guides of p from feat, of a tap q from feat_coarse: n = feat[3..5],
 *      z = feat[6], omc = 1 - feat[7].
 *   4. dot = ((n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z) + omc_p * omc_q
 *      wn = min(1, max(0, dot)), squared normal_pow2 times
 *      wz = 1 where z_p and z_q are both +inf, 0 where exactly one is, else
 *           r = |z_p - z_q| / ((sigma_z * float(s)) * min(z_p, z_q)),
 *           wz = 1 / (1 + r * r)
 *      w = (b * wn) * wz
 *   5. Irradiance of tap q, half h, channel c:
 *      i = half_h[q].c / max(feat_coarse[q].c, 2^-10)
 *   6. In tap order, from 0:  acc_h.c += w * i,  wsum += w.
 *   7. If !(wsum >= 2^-10): step 6 again with w = b (a thin feature that no
 *      coarse pixel agrees with; the b of the taps inside the image sum to at
 *      least 1/4, so wsum > 0 afterwards).
 *   8. out_h.c = (acc_h.c / wsum) * max(feat[p].c, 2^-10).
 *
 * To know: the weights depend on the guides only, so the two outputs stay
 * estimates from disjoint sample sets; but neighbouring output pixels share
 * coarse samples, so rt_denoise's variance, which takes its taps as
 * independent, is understated.  What the features cannot see
 * -- a shadow's edge, a reflection, what lies behind glass -- comes back at
 * the coarse resolution.
 *
 * The inputs are never written.  An output may not overlap an input or the
 * other output (RT_E_ARG); RT_E_ARG too on a NULL required pointer, width or
 * rows <= 0 or more than 2^31 - 1 pixels.  Values other than the library's own
 * (NaN, a depth <= 0) give unspecified numbers, never an out-of-bounds access,
 * a fault or a hang. */
typedef struct rt_upsample_opts {
  int scale, normal_pow2;
  float sigma_z;
} rt_upsample_opts;
/* Asynchronous: one kernel enqueued on hip_stream (NULL: the default stream)
 * of the device that holds d_out0.  All pointers are device pointers, aligned
 * as floats.  Beyond the errors above: RT_E_ARG for more than 4 x 65535 rows
 * or a stream of another device, RT_E_NODEV without a device. */
int rt_upsample(const rt_upsample_opts* o, const float* d_half0, const float* d_half1, const float* d_feat_coarse,
                const float* d_feat, int width, int rows, float* d_out0, float* d_out1, void* hip_stream);
/* The same on the host, in plain C++ (no device; raytracing.clj:141-155): the
 * yardstick of the kernel. */
int rt_upsample_host(const rt_upsample_opts* o, const float* half0, const float* half1, const float* feat_coarse,
                     const float* feat, int width, int rows, float* out0, float* out1);

/* ---- temporal accumulation: history reprojected through first-hit depth -------
 * What a sequence of low-sample frames of compute-pixel's loop
 * (raytracing.clj:141-155) keeps from one frame to the next: per pixel, the
 * accumulated colour of the frames already drawn, fetched from where the
 * pixel's surface point was in the previous frame (found through
 * rt_feat_resolve's depth and the two cameras) if the previous frame saw the
 * same surface there, and blended with the current sample -- the temporal half
 * of SVGF (Schied et al. 2017), between the resolves and rt_denoise.  The two
 * half-frames are accumulated separately: half 0's history only ever receives
 * half-0 samples, so the halves stay independent estimates and rt_denoise's
 * variance term (0.25 d) d shrinks on its own as the history builds.  As the
 * denoiser, a fixed sequence of single fp32 operations, each rounded once in
 * the order written (no fma; / and sqrt IEEE), which the device kernel,
 * rt_temporal_host and a NumPy restatement (tests/test_temporal_host.py) give
 * bit for bit, whatever the workgroup shape.
 *
 * Image: rows x width, contiguous; image row y is camera row row0 + y.  A
 * contiguous row band may be filtered on its own; taps outside the band count
 * as outside the image.
 * Inputs per step: half0, half1 (rows x width x 3 floats each) and feat (rows x
 * width x 8 floats) as for rt_denoise, and the camera that drew them.
 * Options (NULL: the defaults; outside the ranges: RT_E_ARG):
 *   max_history  32    1..65536        cap on the history length
 *   sigma_z      0.1   finite > 0      relative depth tolerance
 *   normal_min   0.9   finite, -1..1   least normal dot product accepted
 * History, per pixel: a0, a1 the accumulated halves (rgb each), g = (n_x, n_y,
 * n_z, z) the guides of the frame that wrote them, and a length L >= 0 as a
 * float (0: none); and a copy of the previous camera (primed below).
 *
 * Host set-up, once per step, in double on the previous camera's fp32 fields,
 * widened:
 *   q = p00' - center'
 *   c0 = dv' x q, c1 = q x du', c2 = du' x dv'  ((a x b)_x = a_y b_z - a_z b_y
 *   and cyclic), det = du' . c0 summed as (x + y) + z,
 *   R_k = c_k / det, each component rounded once to fp32 (k = 0, 1, 2).
 * A det that is 0 or not finite: RT_E_ARG.  dc = center - center' per
 * component in fp32.
 *
 * Per pixel (x, y), j = row0 + y:
 *   1. e_c = ((p00_c + float(x) * du_c) + float(j) * dv_c) - center_c  (the pixel
 *      centre's pinhole ray; the lens jitter is ignored, see below).
 *   2. z_p = feat[6].  If z_p is finite: len = sqrt((e_x^2 + e_y^2) + e_z^2),
 *      sc = z_p / len, w_c = sc * e_c + dc_c, zexp = sqrt((w_x^2 + w_y^2) + w_z^2).
 *      Otherwise (sky): w = e, zexp = +inf.
 *   3. alpha = (R0_x w_x + R0_y w_y) + R0_z w_z; beta, gamma likewise from R1,
 *      R2.  gamma not > 0: no history.  Else fx = alpha / gamma,
 *      fy = beta / gamma - float(row0); fx not (> -1 and < float(width)), or fy
 *      not (> -1 and < float(rows)): no history.  NaN fails these comparisons;
 *      no float is converted to an integer before them.
 *   4. x0 = floor(fx), tx = fx - x0; tx < 2^-6: tx = 0; else tx > 1 - 2^-6:
 *      x0 += 1, tx = 0.  The same for y.  (A still camera is an exact identity,
 *      and no resampling blur below 1/64 pixel.)
 *   5. Taps (x0 + dx, y0 + dy), dy outer, each 0..1, with
 *      b = (dx ? tx : 1 - tx) * (dy ? ty : 1 - ty); a tap with b == 0 or outside
 *      the image is skipped before any load.  A tap q is valid iff L'_q >= 1,
 *      and both z'_q and zexp are +inf, or both are finite and
 *      |z'_q - zexp| <= sigma_z * zexp and
 *      (n_p.x n'_q.x + n_p.y n'_q.y) + n_p.z n'_q.z >= normal_min
 *      (n_p = feat[3..5]).  Over the valid taps, in tap order, from 0:
 *      acc0_c += b * a0'_q.c, acc1_c += b * a1'_q.c, accL += b * L'_q, bsum += b.
 *   6. History is accepted iff bsum >= 0.25: h0 = acc0 / bsum, h1 = acc1 / bsum,
 *      Lh = accL / bsum, N = min(Lh + 1, float(max_history)), k = 1 / N,
 *      out0_c = h0_c + k * (half0_c - h0_c), out1_c likewise.  Without history
 *      out = half and N = 1.
 *   7. a0 = out0, a1 = out1, g = feat[3..6], L = N are stored; the current
 *      camera becomes the previous one.
 * The first step after create or reset has no history (L' = 0 everywhere): it
 * returns its inputs.
 *
 * To know: glass and mirrors are reprojected as their first surface, so what
 * they show lags the camera (rt_temporal_step_clamp, below, bounds that lag by
 * the current frame's colours); the depth is rt_feat's nearest hit over jittered,
 * defocused rays, used as if through the pinhole pixel centre -- that error is
 * what sigma_z absorbs; colour is accumulated modulated, so texture is
 * bilinearly resampled under motion (the scenes here have one albedo per
 * body); rt_temporal_step takes the scene as static between frames -- a body
 * that moved is reprojected as if it had stood still, and on a body of one
 * albedo the depth and normal tests mostly let that pass: for moving bodies
 * use rt_temporal_step_motion (below) with rt_launch_ids and rt_body_motion;
 * and the sample indices of successive frames must differ (the caller's
 * sample_begin or seed), or the history repeats one estimate.
 *
 * The inputs are never written.  Outputs may not overlap inputs or each other
 * (RT_E_ARG).  Inputs are expected as the library produces them; other values
 * -- NaN colours, a depth <= 0, cameras far apart -- give unspecified numbers,
 * never an out-of-range index, a fault or a hang.  A failed call leaves the
 * state, the previous camera included, unchanged. */
typedef struct rt_temporal_opts {
  int max_history;
  float sigma_z, normal_min;
} rt_temporal_opts;
typedef struct rt_temporal rt_temporal;
/* raytracing.clj:141-155's frames, one after another: the history of rows x
 * width images whose first row is camera row row0, on `device`, empty.  It
 * owns two history sets -- a step gathers from the old one while it writes the
 * new -- of three 16-byte words a pixel each: (a0 rgb, L), (a1 rgb, 0) and the
 * guides.  RT_E_ARG on width or rows <= 0, more than 2^31 - 1 pixels or a
 * negative row0, RT_E_NODEV on a device that is not there. */
int rt_temporal_create(int device, int width, int rows, int row0, rt_temporal** out);
int rt_temporal_free(rt_temporal* t);   /* NULL: 0 */
/* raytracing.clj:141-155's loop from its start: forget the history (L = 0
 * everywhere, enqueued on hip_stream) and the previous camera. */
int rt_temporal_reset(rt_temporal* t, void* hip_stream);
/* Steps since the last reset (raytracing.clj:141-155's frame counter); -1 on NULL. */
int64_t rt_temporal_frames(const rt_temporal* t);
/* One step (raytracing.clj:141-155, per frame).  Asynchronous, on hip_stream
 * (NULL: the default stream) of t's device: d_out0, d_out1 (device, rows x
 * width x 3 floats each) = the accumulated halves, which are also the new
 * history.  d_half0, d_half1, d_feat are device pointers, aligned as floats.
 * Steps of one object go on one stream, or are ordered by the caller.
 * RT_E_ARG on a NULL argument, bad options, a degenerate previous camera, an
 * output overlapping an input or the other output, or a stream of another
 * device. */
int rt_temporal_step(rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam, const float* d_half0,
                     const float* d_half1, const float* d_feat, float* d_out0, float* d_out1, void* hip_stream);
/* The current history copied out behind hip_stream's work (tests, checkpoints;
 * raytracing.clj:141-155's state): host_a0, host_a1 (rows x width x 3 floats),
 * host_guide (rows x width x 4), host_len (rows x width); any may be NULL.
 * Returns when they are there. */
int rt_temporal_read(const rt_temporal* t, float* host_a0, float* host_a1, float* host_guide, float* host_len,
                     void* hip_stream);
/* The same step on the host, in plain C++ (no device; raytracing.clj:141-155):
 * the yardstick of the kernel.  prev_cam == NULL: no history (the prev_ arrays
 * are not read); else prev_a0, prev_a1, prev_guide, prev_len are the history
 * in rt_temporal_read's layout.  out0, out1 (rows x width x 3) and out_len
 * (rows x width) are the new history's a0, a1 and L; its guides are
 * feat[3..6]. */
int rt_temporal_host(const rt_temporal_opts* o, const rt_camera* cam, const rt_camera* prev_cam, int width, int rows,
                     int row0, const float* half0, const float* half1, const float* feat, const float* prev_a0,
                     const float* prev_a1, const float* prev_guide, const float* prev_len, float* out0, float* out1,
                     float* out_len);

/* ---- moving bodies: the step with a per-body displacement -----------------------
 * raytracing.clj:141-155's frames when raytracing.clj:63-78's bodies move
 * between them.  The definition above changes in step 2 only.  Two more inputs:
 * ids (rows x width int32, as rt_launch_ids writes them for the current scene
 * and camera) and motion (n_bodies x 4 floats, as rt_body_motion(current scene,
 * previous scene) writes them).
 *   2'. For a finite z_p let b = ids[p]; m = motion[4 b .. 4 b + 2] if
 *       0 <= b < n_bodies, else (0, 0, 0) -- the range test is on the integer,
 *       before any load of the table.  Then w_c = (sc * e_c + dc_c) - m_c (one
 *       more fp32 subtraction), zexp from that w.  A sky pixel (z_p not finite)
 *       ignores ids.
 * Steps 1 and 3-7 are unchanged.  x - (+0) is x for every x, so an all-zero
 * table, ids of -1 or n_bodies = 0 give rt_temporal_step's bits.  Both entries
 * work on the same rt_temporal and may alternate.
 *
 * To know: a NaN displacement (a body rt_body_motion found changed) fails
 * gamma > 0, so the pixel has no history; only rigid translation is followed
 * (rotation of a sphere of one albedo is invisible); shadows, reflections and
 * what glass shows of a moving body lag, as they already do under camera
 * motion, bounded by max_history (rt_temporal_step_clamp, below, clamps such
 * history to the current frame's colour range); and the id is the pinhole centre's body
 * while the depth is rt_feat's nearest hit over jittered rays, so on a
 * silhouette pixel the two can belong to different bodies -- the depth and
 * normal tests are what catch that.
 *
 * rt_temporal_step's arguments and errors, plus RT_E_ARG on a NULL d_ids,
 * n_bodies < 0, a NULL d_motion with n_bodies > 0, a d_motion that is not
 * 16-byte aligned (the kernel loads a row as one word), and an output
 * overlapping d_ids or d_motion.  ids outside 0 .. n_bodies - 1, NaN or huge
 * displacements give "no displacement" or "no history", never an out-of-range
 * index.  A failed call leaves the history and the previous camera unchanged. */
int rt_temporal_step_motion(rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam, const float* d_half0,
                            const float* d_half1, const float* d_feat, const int32_t* d_ids, const float* d_motion,
                            int n_bodies, float* d_out0, float* d_out1, void* hip_stream);
/* The same step on the host, in plain C++ (no device; raytracing.clj:141-155):
 * rt_temporal_host's arguments with ids, motion and n_bodies before the
 * outputs (no alignment is asked of motion here). */
int rt_temporal_host_motion(const rt_temporal_opts* o, const rt_camera* cam, const rt_camera* prev_cam, int width,
                            int rows, int row0, const float* half0, const float* half1, const float* feat,
                            const float* prev_a0, const float* prev_a1, const float* prev_guide, const float* prev_len,
                            const int32_t* ids, const float* motion, int n_bodies, float* out0, float* out1,
                            float* out_len);

/* ---- the colour clamp: stale history held to the current frame's colour range ----
 * raytracing.clj:141-155's frames when what a surface shows changes while the
 * surface itself stays: the steps above ask whether the surface under a pixel
 * is the one the history saw, never whether its shading still is.  Here the
 * fetched history is clamped to a box of the current frame's colours around
 * the pixel before the blend (Karis 2014; Salvi 2016, variance clipping).
 * Options (NULL: the defaults; outside the ranges: RT_E_ARG):
 *   radius  2    1..3            the window is (2 radius + 1)^2 pixels
 *   gamma   1.0  > 0, may be +inf   half the box's width in sample deviations
 *
 * Colour box, per pixel p = (x, y) of the band, from the current half0, half1
 * and feat only (z = feat[6], n = feat[3..5]; sigma_z and normal_min are the
 * step's rt_temporal_opts):
 *   1. Taps (dy, dx), each -radius..radius, dy outer, at q = p + (dx, dy); a
 *      tap outside the band is skipped before any load.  The centre tap is
 *      always valid.  Any other tap is valid iff z_p and z_q are both +inf, or
 *      both are finite and |z_q - z_p| <= sigma_z * z_p and
 *      (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= normal_min.
 *   2. Over the valid taps in tap order, for half k = 0 then 1, per channel c,
 *      from 0: s1_c += v, s2_c += v * v (v = half_k[q].c); once per half,
 *      cnt += 1 (a float).
 *   3. mean_c = s1_c / cnt, var_c = s2_c / cnt - mean_c * mean_c,
 *      var_c = var_c > 0 ? var_c : 0, sd_c = sqrt(var_c), e_c = gamma * sd_c,
 *      lo_c = mean_c - e_c, hi_c = mean_c + e_c.
 * Step 6 with the clamp: after h0_c = acc0_c / bsum and h1_c = acc1_c / bsum,
 *   h0_c = h0_c < lo_c ? lo_c : (h0_c > hi_c ? hi_c : h0_c), the same for h1_c
 * with the same box; the blend, N and the stored L are unchanged.  Pixels
 * without accepted history do not read the box.  Every line is one fp32
 * operation rounded once (no fma; / and sqrt IEEE), as above.
 * gamma = +inf: e is +inf where sd > 0 and NaN where sd == 0; either way both
 * comparisons are false, so the step's bits are rt_temporal_step's (d_ids ==
 * NULL) or rt_temporal_step_motion's for every input.
 *
 * To know: both halves are clamped to one box, so on clamped pixels their
 * difference -- rt_denoise's variance -- is understated; the box is gamma
 * sample deviations wide, so a change smaller than the frame's own noise (a
 * soft sky-light shadow at 2 + 2 spp) is not caught; near silhouettes the
 * window keeps few taps and the box is loose.
 *
 * rt_temporal_step_clamp (raytracing.clj:141-155, per frame): with d_ids ==
 * NULL rt_temporal_step's reprojection, arguments and errors (d_motion and
 * n_bodies are not read); otherwise rt_temporal_step_motion's; plus RT_E_ARG on
 * a radius outside 1..3 or a gamma that is NaN or <= 0.  The first clamp step
 * of an rt_temporal allocates its box scratch, 32 bytes a pixel (RT_E_HIP if
 * that fails); a step with history enqueues the box kernel and then the step
 * kernel on hip_stream.  A failed call leaves the history and the previous
 * camera unchanged.  All three step entries work on one rt_temporal and may
 * alternate. */
typedef struct rt_temporal_clamp_opts {
  int radius;
  float gamma;
} rt_temporal_clamp_opts;
int rt_temporal_step_clamp(rt_temporal* t, const rt_temporal_opts* o, const rt_temporal_clamp_opts* k,
                           const rt_camera* cam, const float* d_half0, const float* d_half1, const float* d_feat,
                           const int32_t* d_ids, const float* d_motion, int n_bodies, float* d_out0, float* d_out1,
                           void* hip_stream);
/* The same step on the host, in plain C++ (no device; raytracing.clj:141-155):
 * rt_temporal_host_motion's arguments with k after o; ids == NULL:
 * rt_temporal_host's reprojection (motion and n_bodies are not read). */
int rt_temporal_host_clamp(const rt_temporal_opts* o, const rt_temporal_clamp_opts* k, const rt_camera* cam,
                           const rt_camera* prev_cam, int width, int rows, int row0, const float* half0,
                           const float* half1, const float* feat, const float* prev_a0, const float* prev_a1,
                           const float* prev_guide, const float* prev_len, const int32_t* ids, const float* motion,
                           int n_bodies, float* out0, float* out1, float* out_len);

/* ---- the sample budget: samples where the temporal history is short ---------------
 * raytracing.clj:141-155's frames when the samples of a frame are not spread
 * evenly: a pixel that carries 32 frames of history gains little from the
 * samples a pixel disoccluded this frame needs badly.  Four parts: the probe
 * asks, before anything is traced, how much history the coming step will
 * accept per pixel; the plan turns that into a sample multiplier per 8 x 8 tile;
 * rt_budget traces the plan into two half accumulators with one read-back per
 * frame; and the weighted step tells the history that a tile's halves hold
 * `mult` frames' worth of samples, so that the next blend weights them so.
 *
 * 1. The probe.  Per pixel, from the *coming* frame's features, ids and motion,
 * the camera that drew them, and t's current history and previous camera:
 * steps 1-5 of the step above (2' when d_ids != NULL, the plain step 2
 * otherwise; sigma_z and normal_min from the same rt_temporal_opts), then
 *   len = accL / bsum if the pixel has history and bsum >= 0.25, else 0.
 * With no previous camera (the first step after create or reset) len = 0
 * everywhere.  Colours are never loaded: of the history only L and the guides
 * of the taps with L >= 1 are read.  It is the step's own text, so for any
 * later step on the same inputs the stored length is min(len + wt,
 * max_history) bit for bit (wt = 1: N).  Nothing is modified.
 *
 * rt_temporal_probe (raytracing.clj:141-155, before a frame): asynchronous, on
 * hip_stream of t's device; d_len (device, rows x width floats) is written,
 * every element.  rt_temporal_step_motion's errors: a NULL argument (d_ids may
 * be NULL: then d_motion and n_bodies are not read), bad options, n_bodies < 0,
 * a NULL or not 16-byte aligned d_motion with n_bodies > 0, d_len overlapping
 * an input, a stream of another device, a degenerate previous camera.  A
 * failed call changes nothing. */
int rt_temporal_probe(const rt_temporal* t, const rt_temporal_opts* o, const rt_camera* cam, const float* d_feat,
                      const int32_t* d_ids, const float* d_motion, int n_bodies, float* d_len, void* hip_stream);
/* The same on the host, in plain C++ (no device; raytracing.clj:141-155):
 * rt_temporal_host_motion's arguments without the halves, prev_a0, prev_a1 and
 * the colour outputs.  prev_cam == NULL: out_len = 0 (prev_guide and prev_len
 * are not read).  ids == NULL: the plain reprojection. */
int rt_temporal_host_probe(const rt_temporal_opts* o, const rt_camera* cam, const rt_camera* prev_cam, int width,
                           int rows, int row0, const float* feat, const float* prev_guide, const float* prev_len,
                           const int32_t* ids, const float* motion, int n_bodies, float* out_len);

/* 2. The plan.  From any rows x width float length image, a multiplier
 * mult[ty * gx + tx] in 1 .. max_mult per 8 x 8 tile of the band; tiles as
 * rt_adapt's: gx = ceil(width / 8), gy = ceil(rows / 8), row-major; a tile's
 * pixels are those inside the band, npx of them.
 * Options (no defaults for half_spp; outside the ranges: RT_E_ARG):
 *   half_spp     -    >= 1     samples of one block: a tile gets 2 mult blocks
 *   target       8    1..32    frames of history a tile is brought up to
 *   max_mult     8    1..16    cap on the multiplier
 *   quantile_64  16   1..64    the share of a tile's pixels, in 64ths, that decides
 * and 2 * max_mult * half_spp <= RT_MAX_SPP.
 * Rule, all in integers: for j = 1 .. target, c_j = the number of the tile's
 * pixels with !(len >= float(j)) (a NaN counts as short); j* = the smallest j
 * with c_j * 64 >= quantile_64 * npx; mult = min(max(target - (j* - 1), 1),
 * max_mult); if no j qualifies, mult = 1.  In words: a tile gets what brings
 * the shortest quantile_64 / 64 of its pixels up to `target` frames.
 * rt_budget_plan_host (raytracing.clj:141-155, before a frame; plain C++, no
 * device): mult (gy x gx) from len.  RT_E_ARG on a NULL argument, bad options,
 * width or rows <= 0. */
typedef struct rt_budget_opts {
  int half_spp, target, max_mult, quantile_64;
} rt_budget_opts;
int rt_budget_plan_host(const rt_budget_opts* o, const float* len, int width, int rows, uint32_t* mult);

/* 3. The budgeted frame.  An rt_budget owns two u64 sum buffers H0 and H1 in
 * rt_adapt's layout, the per-tile mult and counts (= 2 mult half_spp), one
 * device list of all tiles by descending mult (the order among equal
 * multipliers is unspecified: no bit depends on it) and, in page-locked host
 * memory, the prefix counts n_j = #{tiles with mult > j}, j = 0 .. max_mult - 1
 * (n_0 = every tile), the frame's only read-back.
 * Contract: after rt_budget_trace every tile of H0 + H1 equals, integer for
 * integer, that tile of one rt_launch_accum at spp = 2 mult half_spp from
 * p->sample_begin, and H_h is the sum of that tile's sample blocks 2 j + h
 * (block b: indices sample_begin + b half_spp ...), j = 0 .. mult - 1.
 * max_mult = 1 gives two uniform accumulators of half_spp each.
 * To know: the first frame of a sequence has no history and is planned at
 * min(target, max_mult) everywhere -- plan it with rt_budget_plan_mult and ones
 * to avoid that; successive frames must advance sample_begin by 2 max_mult
 * half_spp.
 *
 * rt_budget_create (raytracing.clj:141-155, the loop's state): for frames of
 * `shape` (read and checked as rt_accum_create does) on ds's device; it holds
 * no reference to ds.  RT_E_ARG on a NULL argument, bad options, a tile_step
 * other than 0 (the band must be contiguous) or more than 65535 rows. */
typedef struct rt_budget rt_budget;
int rt_budget_create(const rt_dscene* ds, const rt_params* shape, const rt_budget_opts* opts, rt_budget** out);
int rt_budget_free(rt_budget* bd);   /* NULL: 0 */
/* raytracing.clj:141-155, a frame's start: on hip_stream, H0 = H1 = 0, the plan
 * kernels on d_len (device, rows x width floats, as rt_temporal_probe writes
 * them) and the read-back of the n_j.  Asynchronous. */
int rt_budget_plan(rt_budget* bd, const float* d_len, void* hip_stream);
/* The same from the caller's own gy x gx uint32 multipliers on the device (an
 * importance or foveation map): the values are clamped to 1 .. max_mult on the
 * device before anything indexes by them. */
int rt_budget_plan_mult(rt_budget* bd, const uint32_t* d_mult, void* hip_stream);
/* raytracing.clj:141-155's samples, as planned: waits for the plan's read-back,
 * then for pass j = 0 .. max_mult - 1 with n_j > 0 and half h = 0, 1 enqueues
 * rt_adapt_step's kind of pass over the list's first n_j tiles into H_h, with
 * spp = half_spp and sample indices p->sample_begin + (2 j + h) half_spp ...;
 * p->spp is ignored.  Returns the number of launches.  RT_E_ARG without a
 * fresh plan (one trace per plan), when ds's device or p's shape differ from
 * bd's, when p->sample_begin + 2 max_mult half_spp would pass 2^31 - 1, or when
 * the variant has no 8 x 8 tiles (rt_adapt_step's rule); the frame and the plan
 * are unchanged then.  The stream's tile-cost record (rt_set_schedule) is
 * neither read nor written.  d_counters as rt_launch_accum's. */
int rt_budget_trace(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_budget* bd, uint64_t* d_counters,
                    void* hip_stream);
/* raytracing.clj:141-155's samples, as planned, in two launches: rt_budget_trace's
 * arguments, checks, refusals and contract -- afterwards H0 and H1 each hold,
 * integer for integer, what rt_budget_trace leaves on the same plan, and
 * d_counters receives the same {segments, samples}.  It waits for the plan's
 * read-back as rt_budget_trace does, then enqueues a kernel that writes, per
 * half h, a table of U = sum_j n_j units on the device,
 *   slot sum_{j' < j} n_j' + i:  {tile = list[i], (2 j + h) | (2 max_mult) << 8},
 * for j = 0 .. max_mult - 1 and list positions i < n_j (block-major, in list
 * order: pass 0's tiles, then pass 1's, ...), and one pass per half over its
 * table: U workgroups, unit {tile, k | s << 8} tracing samples [k spp / s,
 * (k + 1) spp / s) of the tile with spp = 2 max_mult half_spp -- block k of
 * half_spp samples, indices p->sample_begin + k half_spp ....  The kernel picks
 * the width of its pixel sums from that total spp, not from half_spp: this
 * changes the variant's internals, not the bits.  Returns the number of trace
 * launches, 2.  The tables (n_tiles x max_mult x 8 bytes per half) are
 * allocated by the first call. */
int rt_budget_trace_fused(const rt_dscene* ds, const rt_camera* c, const rt_params* p, rt_budget* bd,
                          uint64_t* d_counters, void* hip_stream);
/* The unit table of half `half` (0 or 1) on the host, in plain C++ (no device;
 * raytracing.clj:141-155, before a frame): from `list` (every tile 0 .. n_tiles -
 * 1 once, by descending multiplier) and mult (n_tiles values in 1 .. max_mult),
 * units receives sum_t mult[t] entries of two int32 each, as above; returns
 * their number.  RT_E_ARG, with nothing written, on a NULL argument, n_tiles <=
 * 0, max_mult outside 1..16, a half other than 0 or 1, a multiplier outside
 * 1 .. max_mult, or a list that is no permutation of the tiles in descending
 * order of multiplier. */
int rt_budget_units_host(const int32_t* list, const uint32_t* mult, int n_tiles, int max_mult, int half,
                         int32_t* units);
/* raytracing.clj:141-155's plan as traced: the device's table of half `half`
 * copied to host_units (room for n_tiles x max_mult entries of two int32 is
 * always enough); returns the number of entries U.  RT_E_ARG when no
 * rt_budget_trace_fused has run since the last plan.  And the device's list
 * (n_tiles int32: every tile, by descending multiplier) of the current plan.
 * Both return when the data is there. */
int rt_budget_units_read(const rt_budget* bd, int half, int32_t* host_units, void* hip_stream);
int rt_budget_list_read(const rt_budget* bd, int32_t* host_list, void* hip_stream);
/* compute-pixel's accum / spp per tile (raytracing.clj:155): rt_adapt_resolve's
 * and rt_adapt_resolve_half's conversions with this frame's counts. */
int rt_budget_resolve(const rt_budget* bd, int flags, float* d_out, void* hip_stream);
int rt_budget_resolve_half(const rt_budget* bd, int half, int flags, float* d_out, void* hip_stream);
/* raytracing.clj:141-155's accum, both halves, as rt_adapt_read; the gy x gx
 * multipliers of the current plan copied to host_mult; and where they lie on
 * the device (for rt_temporal_step_budget; valid until rt_budget_free, rewritten
 * by the next plan).  The reads return when the data is there. */
int rt_budget_read(const rt_budget* bd, uint64_t* host_sums0, uint64_t* host_sums1, void* hip_stream);
int rt_budget_mult_read(const rt_budget* bd, uint32_t* host_mult, void* hip_stream);
int rt_budget_device_mult(const rt_budget* bd, const uint32_t** d_mult);
/* raytracing.clj:141-155's counter: the sum over the tiles of npx * 2 * mult *
 * half_spp of the current plan (waits for its read-back); 0 before a plan. */
int64_t rt_budget_samples(rt_budget* bd);

/* 4. The weighted step.  rt_temporal_step_clamp with d_mult (device, gy x gx
 * uint32: the tiles of the band as above) after n_bodies.  Per pixel (x, y),
 *   wt = float(min(max(mult[(y / 8) * gx + x / 8], 1), 16)),
 * and step 6 becomes: with history N = min(Lh + wt, float(max_history)),
 * k = wt / N; without history out = half and N = min(wt, float(max_history)).
 * Everything else is unchanged: steps 1-5, the clamp, 2' with ids, and what is
 * stored.  With every multiplier 1 the bits are rt_temporal_step_clamp's:
 * 1.0f / N and Lh + 1.0f are the same operations.  With gamma = +inf no box
 * kernel is enqueued (the bits are equal, as shown above).  L now counts
 * base-frame equivalents, which is what the plan's `target` is measured in.
 * rt_temporal_step_clamp's errors, plus RT_E_ARG on a NULL d_mult or an output
 * overlapping it (raytracing.clj:141-155, per frame). */
int rt_temporal_step_budget(rt_temporal* t, const rt_temporal_opts* o, const rt_temporal_clamp_opts* k,
                            const rt_camera* cam, const float* d_half0, const float* d_half1, const float* d_feat,
                            const int32_t* d_ids, const float* d_motion, int n_bodies, const uint32_t* d_mult,
                            float* d_out0, float* d_out1, void* hip_stream);
/* The same step on the host, in plain C++ (no device; raytracing.clj:141-155):
 * rt_temporal_host_clamp's arguments with mult (gy x gx) after n_bodies. */
int rt_temporal_host_budget(const rt_temporal_opts* o, const rt_temporal_clamp_opts* k, const rt_camera* cam,
                            const rt_camera* prev_cam, int width, int rows, int row0, const float* half0,
                            const float* half1, const float* feat, const float* prev_a0, const float* prev_a1,
                            const float* prev_guide, const float* prev_len, const int32_t* ids, const float* motion,
                            int n_bodies, const uint32_t* mult, float* out0, float* out1, float* out_len);

/* ---- moving bodies: an uploaded scene updated in place --------------------------
 * raytracing.clj:63-78's bodies at new centres, without a new rt_scene_upload:
 * the scene's trees keep their topology and are refitted on the device.
 *
 * rt_scene_update: sphere is a host array of ds's n x 4 floats (centre, radius)
 * in body order; the scene's materials, kinds and radii stay.  After the call,
 * in the order of hip_stream (NULL: the default stream), the scene on the
 * device is what rt_scene_upload would have made of the new spheres had its
 * builder kept the upload's topology: which bodies are out of the tree, which
 * are big, each leaf's bodies, each node's children.
 *
 * Preconditions; any violation returns RT_E_ARG and nothing on the device or
 * in ds has changed:
 *   - no argument is NULL (a NULL sphere is allowed when n == 0);
 *   - every radius equals the upload's bit for bit (so the median, the big
 *     list, r_max, c0, -r^2, 1/r and the Schlick terms stay valid);
 *   - for every body whose r * r is finite, "all three centre coordinates are
 *     finite" is what it was at the upload: a body in the tree or the big list
 *     cannot leave it, one left out for its centre cannot join; a body left
 *     out for its radius may have any centre;
 *   - hip_stream is a stream of ds's device.
 * The scene keeps a host copy of the upload's spheres to check this.
 *
 * Tables: geo[i] and its pair-interleaved copy get body i's new centre (and
 * the same -r^2); sph[i] its new centre, the 1/r lane untouched.  Every leaf
 * record slot that holds a body (the tree's leaves and the big bodies') gets
 * that body's x, y, z; w, the pads, the indices, materials and kinds are not
 * written.
 * Per tree k in {0, 1, 2}: centre and radius come by the build's own formula
 * over the tree's bodies (the centre of their box; the farthest surface from
 * it, in double, x (1 + 1e-6) + 1e-6), on the host inside the call: they are
 * launch arguments, stored in ds on return, so a launch enqueued after the
 * call carries the new ones and one enqueued before it carried the old.
 * Per tree k, node and child: B = the union over the bodies under that child
 * of the body's box (per axis c -+ |r|, one fp32 operation, then one step
 * outward); each stored bound is float(double(B.lo) - double(centre)) stepped
 * once towards -inf, the max plane likewise towards +inf, the third pair a
 * copy of the first.  A tree without bodies has B = the point 0 for both root
 * children; a tree of one leaf has that leaf under both.  Child refs are not
 * written.  Min and max are exact, so the bytes do not depend on the order of
 * evaluation: an update with the upload's own spheres changes no byte, and
 * the device's bytes are rt_tree_refit_host's.
 *
 * Ordering: the work is enqueued on hip_stream and the call does not wait for
 * it; sphere may be reused as soon as the call returns (the scene copies it to
 * page-locked staging of its own; the fifth update in flight waits for the
 * first's copy).  Work on the same stream sees the scene before or after the
 * update, by its place in the stream.  Work already enqueued on *other*
 * streams that reads this scene races with the update, as work on another
 * stream does with rt_accum's buffers: order it yourself.  Calls on one scene
 * are not to run concurrently with one another or with launches on it from
 * other threads.  A failed device call leaves ds's host scalars at their old
 * values.  The tile-cost records of the adaptive order (rt_set_schedule), the
 * scene's id and its allocations are kept.
 * To know: the refitted tree is as tight as its topology allows, not as a
 * fresh build would be; rt_tree_cost_host tells how far it has loosened.  A
 * change of radius, material, kind or body count needs a fresh upload. */
int rt_scene_update(rt_dscene* ds, const float* sphere, void* hip_stream);

/* One tree of a scene as the device holds it: blob = nodes | pairs | pidx.
 * Nodes are 80 bytes: the two child boxes as x[6], y[6], z[6] floats -- per
 * axis (min0, min1, max0, max1, min0, min1), relative to center -- and two int
 * child refs (>= 0 an inner node: its index, or for the 4-body tree its byte
 * offset; < 0 a leaf: ~ its first pair).  Pairs are 8 floats (x0 x1 y0 y1 z0 z1
 * w0 w1, w = -r^2, +inf for a pad); a leaf is leaf_size / 2 consecutive pairs;
 * the big bodies' n_big_leaves leaves start at pair big_pair0.  pidx holds two
 * body indices per pair, idx_bytes each (4: int, -1 a pad; 2: u16, 0xffff a
 * pad), padded to 16 bytes.  Offsets in bytes.  c0: the walk's padding term
 * (3 x the tree bodies' largest |radius|). */
typedef struct rt_tree_info {
  int n_nodes, off_pairs, off_pidx, blob_bytes, big_pair0, n_big_leaves, depth, leaf_size, idx_bytes;
  float center[3], radius, c0;
} rt_tree_info;

/* Host entries (plain C++, no device).  k = 0, 1, 2: the tree of 2-, 4- and
 * 8-body leaves.
 * rt_tree_build_host: exactly the blob rt_scene_upload uploads for tree k of
 * the n bodies `sphere` (n x 4 floats), into blob (cap bytes), described in
 * info.  RT_E_ARG on a NULL sphere (n > 0) or info, bad n or k; and when cap
 * is too small (blob may then be NULL): info is filled, blob_bytes is the size
 * needed, blob is not written. */
int rt_tree_build_host(const float* sphere, int n, int k, void* blob, size_t cap, rt_tree_info* info);
/* rt_scene_update's definition applied to a host blob in place, for one tree:
 * sphere_at_upload is what the blob was built from, sphere_now the new
 * spheres; info's center and radius are updated.  The same preconditions and
 * errors, plus RT_E_ARG for an info or blob that is not a tree over n bodies;
 * on an error the blob and info are unchanged. */
int rt_tree_refit_host(void* blob, rt_tree_info* info, const float* sphere_at_upload, const float* sphere_now, int n);
/* *cost = the sum over nodes and their two children of the child box's surface
 * area 2 (dx dy + dy dz + dz dx), in double, in node order: the figure a
 * surface-area build minimises; its ratio to the value at the upload tells
 * how far refits have loosened a tree. */
int rt_tree_cost_host(const void* blob, const rt_tree_info* info, double* cost);
/* The device's counterparts (tests, tools): tree k of ds as it stands, and
 * its blob copied to the host (cap >= info's blob_bytes) behind hip_stream's
 * work: the call waits for the stream, then copies. */
int rt_scene_tree_info(const rt_dscene* ds, int k, rt_tree_info* info);
int rt_scene_tree_read(const rt_dscene* ds, int k, void* blob, size_t cap, void* hip_stream);

/* Asynchronous: enqueue rt_quantize on hip_stream's device for n channels
 * already in HBM (d_lin: n floats, d_out: n bytes, device pointers): the same
 * bytes as rt_quantize for every float (NaN, infinities and denormals
 * included), through a table of the 255 float thresholds between bytes that
 * the host derives from rt_quantize's own arithmetic. */
int rt_quantize_device(const float* d_lin, uint8_t* d_out, size_t n, void* hip_stream);

/* Kernel variant selector (all variants give identical bits).  The product
 * library holds: 0 = default (22 where it applies, else 16; when the 4-body
 * tree's LDS image would cap a CU below 5 workgroups and the 8-body tree's
 * is smaller: 26 where 22 applies and two of its 16-wave workgroups fit a
 * CU, else 24 where three of its 8-wave workgroups fit, else 18);
 * 16 = BVH traversal, 4 bodies per leaf, nodes and leaf bodies in LDS;
 * 18 = the same with 8 bodies per leaf, in 512-thread workgroups (one LDS
 * image per 8 waves); 22 = 16 in a compact LDS image (u8 node-index stack,
 * u32 pixel sums that count their wraps above 255 spp: seven workgroups per
 * CU; 0 selects it wherever spp < 65536, every albedo lies in [-1, 1], the
 * tree has <= 256 nodes and no frame side exceeds 65536, else 16; a path's
 * camera segment is resolved against a per-tile list of the bodies its
 * tile's camera rays can reach, not by the traversal); 30 = 22 without that
 * list (every segment through the traversal); 24 = 22's
 * image in 512-thread workgroups (one per 8 waves; 16 where 22 does not
 * apply); 26 = the same in 1024-thread workgroups (8 waves per SIMD); 12 = BVH
 * with 2 bodies per leaf read from global memory (the fallback for a tree
 * too big for LDS); 5 = linear scan, bodies in groups of 4 through the
 * scalar cache (the fallback for a tree too deep for the stack).  The
 * diagnostic build lib/librtclj_diag.so (make diag) adds: 1 / 2 = simple
 * scan, table in LDS / scalar cache; 4 = grouped scan, table in LDS
 * (north_star's LDS-staged sphere list); 8 / 9 = packed-fp32 scan, LDS /
 * scalar; 11 = BVH in LDS, 2 bodies per leaf; 20 / 21 = direction-sorted
 * 8-wave lock-step workgroups (octant sort / live-path packing); and the
 * statistics builds 3, 6, 7, 10, 13, 17, 19, 31 (= 1, 4, 5, 9, 11, 16, 18, 22
 * with wave-level counters, rt_debug_stats).  Returns the previous value, or
 * RT_E_ARG for a variant this build does not hold.  Applies to subsequent
 * launches in this
 * process (an atomic, read once per launch). */
int rt_set_variant(int variant);

/* The kernel variant the current selector resolves to for ds (the default
 * resolved for this scene, or a fallback when a tree does not fit), before
 * the per-launch choice of the compact image (16 -> 22, 18 -> 26 / 24), which also
 * depends on the launch (spp < 65536, frame size): rt_launch_occupancy's
 * out4[3] reports the variant a given launch runs.  For reading the matching
 * statistics build.  -1 on a NULL scene. */
int rt_resolve_variant(const rt_dscene* ds);

/* Occupancy of the launch rt_launch would make for (ds, p) under the current
 * selectors (diagnostic): out4 = {256-thread workgroups per CU (HIP occupancy
 * query with the launch's dynamic LDS), VGPRs per lane, LDS bytes per
 * workgroup, the variant}. */
int rt_launch_occupancy(const rt_dscene* ds, const rt_params* p, int* out4);

/* Tile dispatch order of rt_launch.  0 (default) = adaptive: every launch
 * adds how long each 8 x 8 pixel tile's waves ran to half the tile's earlier
 * record, and a one-block sort enqueued after it (same stream, no host sync)
 * turns that into a longest-first order; the next launch on the same scene and stream with the
 * same launch shape (width, row selection; camera, spp, seed, flags and the
 * kernel variant may differ) dispatches its tiles in that order, so the slow
 * tiles do not trail the kernel's end.  A launch of another shape runs in
 * plain order and re-keys the record (per scene, up to 16 streams; launches on
 * further streams are unscheduled).  1 = always plain order.  Changes timing
 * only: every pixel is computed the same way in any order (bit-identical
 * output).  Returns the previous value, RT_E_ARG for another mode. */
int rt_set_schedule(int mode);

/* Diagnostic counters of the stats variants (diagnostic build) since the
 * last call (then cleared), summed over devices, 32 values: [0] wave loop
 * iterations, [1] active lanes summed over them, [2] body tests per wave
 * (scan) / node visits per lane (BVH), [3] candidate blocks per wave (scan) /
 * leaf tests per lane (BVH), [4] lanes in candidate blocks / exact body
 * tests (BVH), [5] waves, [6] BVH wave-level traversal iterations, [7] lanes
 * active in them, [8..11] shader clocks per wave spent in camera sampling,
 * hit search, shading, accumulation (s_memtime; summed over waves), [12] BVH
 * wave-level leaf passes, [13] wave-level exact-test passes, [14] / [15]
 * wave-level trips of the random-unit-vec3 / defocus-disk rejection loops,
 * [16] / [17] wave-level camera-sample blocks / lanes in them, [18] executed
 * fp32 flops (per lane, fma = 2), [19] / [20] wave-level
 * dielectric shading blocks / lanes in them, [21] / [22] wave-level
 * lambertian-or-metal shading blocks / lanes in them, [23..26] wave-level
 * colour-sum blocks, refills, batch claims, drain checks, [27..31] variant
 * 31 (the tile list's prelude): wave-level prelude trips,
 * lanes in them, the trips' list passes (up to four listed bodies each),
 * their exact steps (one per body some lane holds a candidate of; both also
 * in [12] / [13]), walk segments entered in an iteration that ran a trip.
 * Synchronises the devices. */
int rt_debug_stats(uint64_t* out32);
/* The same read-out (and the same clearing) with the counters added since the
 * array was 32 long: the first n of 40 values, n in 0 .. 40.  [32] variant
 * 31: the bodies its list passes tested (four or two a pass, a pass's repeats
 * of a body included); [33..39] unused, 0. */
int rt_debug_stats_ext(uint64_t* out, int n);

/* The camera prelude's list of one tile on the host, in plain C++ (no device;
 * raytracing.clj:33-43 for a tile's camera rays): the bodies of s that
 * variant 22's workgroup prologue lists for 8 x 8 tile `tile` (row-major over
 * the launch's compacted rows, ceil(width / 8) tiles a row) of the launch (c,
 * p) -- csrc/tile_list.h's cull, the text the kernel runs, over the leaf
 * records of the 4-body tree.  bodies receives the first cap kept bodies'
 * indices, in record order (the kernel's order is not defined); slots
 * (nullable) their places, 4 x record + slot.  Returns how many bodies are
 * kept (more than 14: the kernel makes no list for the tile, its camera rays
 * take the walk), 0 for a tile without pixels.  RT_E_ARG on a NULL s, c, p or
 * bodies, a negative cap or tile, or a row selection rt_rows_out refuses. */
int rt_tile_bodies_host(const rt_scene* s, const rt_camera* c, const rt_params* p, int tile, int32_t* bodies,
                        int32_t* slots, int cap);

/* Diagnostic wave timeline of the stats variants' last launches on `device`
 * (of every variant's when the diagnostic build is loaded with
 * RTCLJ_TIMELINE=1):
 * n_waves x {start, end (s_memrealtime, 100 MHz), HW_ID, XCC_ID}; returns
 * the count. */
int rt_debug_waves(int device, uint64_t* out, size_t n_waves);

/* Sample stealing of rt_launch (diagnostic): the launches on (ds, hip_stream)
 * since the last call made out2[0] steals of out2[1] samples in all (a
 * workgroup that finds no tile left to start takes free samples of another
 * workgroup's tile).  Waits for the stream, then clears the
 * counts.  Timing only: the bits never depend on it. */
int rt_steal_stats(const rt_dscene* ds, void* hip_stream, uint64_t* out2);

/* Path export of rt_launch's split launches (diagnostic; RTCLJ_EXPORT=1):
 * out2[0] = the launches on (ds, hip_stream) since the last call that wrote
 * their waves' last paths out for a sweep launch, out2[1] =
 * the records the latest of them wrote.  Waits for the stream.  Timing
 * only: the bits never depend on it. */
int rt_export_stats(const rt_dscene* ds, void* hip_stream, uint64_t* out2);

/* The adaptive order's record of (ds, hip_stream), read out (diagnostic; the
 * tests of the schedule read it).  exists: the stream owns one of the scene's
 * 16 entries (0: its launches run unscheduled, every other field is as
 * below for "none").  n_tiles: the tile count of the launch shape the entry
 * is keyed to (0 before a launch).  has_record: the cost and order buffers
 * hold n_tiles entries.  ready: the order is the sort of a record and the next
 * launch of the shape uses it as it stands.  sort_pending: the last launch
 * added to the record and its sort runs at the start of the next launch of
 * the shape.  plan_units: the unit count of the cost-balanced split plan the
 * last sort made (RTCLJ_SPLIT_PLAN=1; -1: none).  sort_plan: the unit count
 * the pending sort will plan for (-1: none).  max_streams: the streams a scene
 * keeps entries for (16), set whether or not this stream owns one. */
typedef struct rt_schedule_info {
  int32_t exists;
  int32_t n_tiles;
  int32_t has_record;
  int32_t ready;
  int32_t sort_pending;
  int32_t plan_units;
  int32_t sort_plan;
  int32_t max_streams;
} rt_schedule_info;

/* Waits for hip_stream, then copies out the entry's n_tiles per-tile costs
 * (100 MHz ticks: each launch's workgroup durations added to half the record
 * before it), its n_tiles order positions as they stand (order[i] = the tile
 * dispatched i-th) and the plan's plan_units units ({tile, k | s << 8} as two
 * int32 each; {-1, 0}: unused).  host_cost, host_order and host_units may be
 * NULL (info only); cap_tiles and cap_units are their capacities in tiles and
 * in units.  Changes nothing: no pending sort is run, no flag flipped, no
 * buffer grown.  RT_E_ARG for a NULL ds or info, or a cap smaller than what
 * the buffer would receive (a cap of 0 for a buffer that is given, always);
 * nothing is written then.  Timing only: the bits never depend on it. */
int rt_schedule_read(const rt_dscene* ds, void* hip_stream, rt_schedule_info* info, uint32_t* host_cost,
                     int32_t* host_order, int32_t* host_units, int cap_tiles, int cap_units);

/* The schedule's sort on the caller's data, without a scene (diagnostic): the
 * n costs, host_order's n entries and (U > 0) host_units' 2 U int32 go up to
 * `device` as they are; the sort kernel, and for U > 0 the plan kernel with at
 * most smax units per tile, run on hip_stream exactly as a launch enqueues
 * them; then the halved costs, the longest-first order and the U units come
 * back.  Waits for the stream.  RT_E_ARG for a NULL array, n <= 0, U < 0,
 * 0 < U < n, or smax outside 1 .. 64; RT_E_NODEV when `device` is not there. */
int rt_schedule_sort(int device, uint32_t* host_cost_inout, int n, int32_t* host_order, int U, int smax,
                     int32_t* host_units, void* hip_stream);

/* A device's one-time start-up, done ahead of the first render so that a
 * one-frame process (-main, raytracing.clj:95-177) can overlap it with its
 * own work (rt_main starts it on a thread at process start): the device
 * context, the kernels' code object, the NULL stream's hardware queue and
 * the runtime's staging for pageable copies.  out_ms4 (nullable) = the
 * milliseconds of those four steps.  Idempotent; rt_render does the same
 * work lazily when it was not called. */
int rt_prepare(int device, double* out_ms4);

int rt_device_count(void);
const char* rt_last_error(void);
const char* rt_version(void);
int rt_abi_version(void);   /* RT_ABI_VERSION the library was built with */

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* RT_H */
