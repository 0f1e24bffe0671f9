// gv_resources.hpp -- the owning types of the host side: a device buffer, a pinned host buffer, an event, a stream.
// Move-only; the destructor releases and ignores HIP errors (a handle is torn down after its streams were
// synchronised, nothing useful is left to do with a failure there).  Each converts implicitly to the raw HIP
// type, so kernel-argument structs and launch calls take them as they took the raw pointers.
// The calls that can fail take the handle (anything with a std::string `err`), record the HIP error there and
// return GV_ERR_HIP, like GV_HIP does.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstddef>
#include <utility>

#include "../../include/gridvision_hip.h"

namespace gv_internal __attribute__((visibility("hidden"))) {

template <class H>
inline int hip_failed(H *h, hipError_t e, const char *what)
{
  char buf[160];
  std::snprintf(buf, sizeof(buf), "%s -> %s", what, hipGetErrorString(e));
  h->err = buf;
  return GV_ERR_HIP;
}

// A device allocation and its capacity in elements.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept
  {
    if (this != &o) {
      release();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  operator T *() const { return p_; }
  T *get() const { return p_; }
  size_t cap() const { return cap_; }
  void release()
  {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // At least `need` elements: nothing when they are there, otherwise the old block is freed and exactly `need` are
  // allocated (growth slack is the caller's).  On failure the buffer is empty.
  template <class H>
  int reserve(H *h, size_t need)
  {
    if (need <= cap_) return GV_OK;
    release();
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), need * sizeof(T));
    if (e != hipSuccess) {
      p_ = nullptr;
      return hip_failed(h, e, "hipMalloc");
    }
    cap_ = need;
    return GV_OK;
  }
  // For buffers that every user leaves zero: a new block is zeroed on stream s.
  template <class H>
  int reserve_zeroed(H *h, size_t need, hipStream_t s)
  {
    if (need <= cap_) return GV_OK;
    if (int rc = reserve(h, need)) return rc;
    const hipError_t e = hipMemsetAsync(p_, 0, need * sizeof(T), s);
    return e == hipSuccess ? GV_OK : hip_failed(h, e, "hipMemsetAsync");
  }

 private:
  T *p_ = nullptr;
  size_t cap_ = 0;
};

// The same over pinned host memory, in bytes; `flags` are hipHostMalloc's.
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  PinnedBuf &operator=(PinnedBuf &&o) noexcept
  {
    if (this != &o) {
      release();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~PinnedBuf() { release(); }
  operator uint8_t *() const { return p_; }
  uint8_t *get() const { return p_; }
  size_t cap() const { return cap_; }
  void release()
  {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  template <class H>
  int reserve(H *h, size_t need, unsigned flags)
  {
    if (need <= cap_) return GV_OK;
    release();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p_), need, flags);
    if (e != hipSuccess) {
      p_ = nullptr;
      return hip_failed(h, e, "hipHostMalloc");
    }
    cap_ = need;
    return GV_OK;
  }

 private:
  uint8_t *p_ = nullptr;
  size_t cap_ = 0;
};

// An event; create() names its flags (hipEventDefault: a timing event).
class Event {
 public:
  Event() = default;
  Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event &operator=(Event &&o) noexcept
  {
    if (this != &o) {
      release();
      e_ = std::exchange(o.e_, nullptr);
    }
    return *this;
  }
  ~Event() { release(); }
  operator hipEvent_t() const { return e_; }
  hipError_t create(unsigned flags)
  {
    release();
    return hipEventCreateWithFlags(&e_, flags);
  }
  void release()
  {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }

 private:
  hipEvent_t e_ = nullptr;
};

// A non-blocking stream.
class Stream {
 public:
  Stream() = default;
  Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  Stream &operator=(Stream &&o) noexcept
  {
    if (this != &o) {
      release();
      s_ = std::exchange(o.s_, nullptr);
    }
    return *this;
  }
  ~Stream() { release(); }
  operator hipStream_t() const { return s_; }
  hipError_t create()
  {
    release();
    return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
  }
  void release()
  {
    if (s_) (void)hipStreamDestroy(s_);
    s_ = nullptr;
  }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace gv_internal
