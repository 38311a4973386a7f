// launch.h — what a launch site of any unit needs: the HIP error path, the
// typed enqueue, the library's fill (fill_kernel is the trace unit's), the
// quantiser's threshold table, the check of a launch's frame arguments and the
// stream-on-device check.  Included behind the HIP runtime
// header.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

#include "dev_buf.h"
#include "rt_internal.h"

namespace rtclj {

inline int hip_fail(hipError_t e, const char* what) {
  return set_error(RT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(call)                                           \
  do {                                                          \
    hipError_t _e = (call);                                     \
    if (_e != hipSuccess) return ::rtclj::hip_fail(_e, #call);  \
  } while (0)

// A launch of one of the including unit's kernels: each argument converted to
// the kernel's parameter type at compile time (a narrowing one is an error),
// then the pointer array hipLaunchKernel takes.
template <class... P, class... Args>
hipError_t enqueue(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args&&... args) {
  static_assert(sizeof...(P) == sizeof...(Args), "enqueue: the kernel's parameter count");
  const auto launch = [&](P... v) {
    void* ptrs[] = {const_cast<void*>(static_cast<const void*>(&v))...};
    return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, lds, stream);
  };
  return launch(P{std::forward<Args>(args)}...);
}
// ... of a variant-table kernel: one KArgs / FeatArgs by value
template <class A>
hipError_t enqueue(const void* fn, dim3 grid, dim3 block, size_t lds, hipStream_t stream, A& a) {
  void* ptrs[] = {&a};
  return hipLaunchKernel(fn, grid, block, ptrs, lds, stream);
}

// The library's fill (trace.hip): n words of p set to `word` (fill_kernel
// takes any word: +inf's bits for the feature depths)
hipError_t fill_words(void* p, uint32_t word, size_t n, hipStream_t stream);
template <class T>
hipError_t fill_zero(const DevBuf<T>& b, size_t n, hipStream_t stream) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  return fill_words(b.p, 0u, n * (sizeof(T) / 4), stream);
}

// rt_quantize's thresholds (rt_internal.h) as a kernel argument
struct QThr {
  float t[256];
};
inline const QThr& quantize_table() {
  static const QThr thr = [] {
    QThr t;
    std::memcpy(t.t, quantize_thresholds(), sizeof t.t);
    return t;
  }();
  return thr;
}

// an A/B knob of the environment, read where it is used: at least lo, or dflt
inline int env_int(const char* name, int dflt, int lo) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::atoi(e)) : dflt;
}

// The HIP occupancy query on a kernel at a workgroup size and dynamic LDS:
// out4[0..2] = {workgroups per CU, VGPRs per lane, LDS bytes per workgroup}
inline int occupancy_report(const void* fn, int threads, size_t lds, int* out4) {
  int blocks = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, threads, lds));
  hipFuncAttributes fa{};
  HIP_TRY(hipFuncGetAttributes(&fa, fn));
  out4[0] = blocks;
  out4[1] = fa.numRegs;
  out4[2] = static_cast<int>(lds + fa.sharedSizeBytes);
  return RT_OK;
}

// a launch's frame arguments (rt_launch, rt_launch_accum, rt_adapt_step, rt_launch_feat)
inline int check_frame_args(const char* who, const rt_params& p) {
  if (p.width <= 0 || p.height <= 0 || p.spp < 0 || p.spp > RT_MAX_SPP ||
      (p.flags & ~(RT_FLAG_REALM | RT_FLAG_STREAMED | RT_FLAG_REJECTION_SAMPLERS)) != 0)
    return set_error(RT_E_ARG, std::string(who) + ": bad width/height/spp/flags");
  return RT_OK;
}

// nullptr's device, or whether `stream` belongs to the device `noun` ("the
// scene", "the history", ...) is on
inline int stream_on_device(const std::string& me, hipStream_t stream, int device, const char* noun) {
  if (!stream) return RT_OK;
  hipDevice_t sdev = 0;
  if (hipStreamGetDevice(stream, &sdev) == hipSuccess && static_cast<int>(sdev) != device)
    return set_error(RT_E_ARG, me + ": the stream is on device " + std::to_string(static_cast<int>(sdev)) + ", " + noun +
                                   " on device " + std::to_string(device));
  return RT_OK;
}

}  // namespace rtclj
