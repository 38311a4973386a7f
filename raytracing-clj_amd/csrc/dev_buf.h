// dev_buf.h — an owning device buffer: a pointer and its capacity, move-only,
// freed by its destructor.  Included behind the HIP runtime header (launch.h);
// the host check of its move logic includes it behind counting stand-ins for
// hipMalloc / hipFree / hipStreamSynchronize.
#pragma once
#include <cstddef>

namespace rtclj {

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;   // elements

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  explicit operator bool() const { return p != nullptr; }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // n elements in place of what it holds, which no kernel may still use
  hipError_t alloc(size_t n) {
    reset();
    const hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    else p = nullptr;
    return e;
  }
  // at least n elements.  Growing waits for `stream`, whose kernels may still
  // use the old buffer, frees that and allocates; the contents are not kept,
  // and the capacity is set once the allocation has succeeded.  *grew: whether
  // it did (the caller then fills the buffer, resets what described it).
  hipError_t reserve(size_t n, hipStream_t stream, bool* grew = nullptr) {
    if (grew) *grew = false;
    return cap >= n ? hipSuccess : regrow(n, stream, grew);
  }
  // exactly n elements: as reserve, for a buffer whose size the kernel reads
  hipError_t resize(size_t n, hipStream_t stream, bool* grew = nullptr) {
    if (grew) *grew = false;
    return cap == n ? hipSuccess : regrow(n, stream, grew);
  }

 private:
  hipError_t regrow(size_t n, hipStream_t stream, bool* grew) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    e = alloc(n);
    if (e == hipSuccess && grew) *grew = true;
    return e;
  }
};

}  // namespace rtclj
