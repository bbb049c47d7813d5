// hbmem.h — the one owning buffer type of the engine's host side.
//
// Plain C++17, no HIP: the allocation calls come from the Mem traits
// (static void* alloc(size_t bytes), null on failure; static void free(void*)),
// so the type is tested on the CPU alone (tests/asan/hbmem_asan.cpp).
// hipbatch.hip defines the device and the pinned-host traits.
#ifndef HBMEM_H_
#define HBMEM_H_

#include <cstddef>
#include <cstdint>

#include "../../include/hipbatch.h"

namespace hbmem {

// reserve()'s default hook: the old block has no reader left
struct NoWait {
  int operator()() const { return HB_OK; }
};

// A block of cap() elements of T.  Move-only; the destructor frees.
template <class T, class Mem>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
    o.p_ = nullptr;
    o.cap_ = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_;
      cap_ = o.cap_;
      o.p_ = nullptr;
      o.cap_ = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }

  // Room for `need` elements.  Nothing happens while need <= cap().  Otherwise
  // `idle` runs first (the call site's wait for the old block's last reader;
  // a code other than HB_OK is returned as it is and the buffer stays), the
  // old block is freed and max(need, grow_to) elements are allocated: the
  // contents are not kept.  HB_ENOMEM leaves the buffer empty.
  template <class Idle = NoWait>
  int reserve(uint64_t need, uint64_t grow_to = 0, Idle&& idle = Idle()) {
    if (need <= cap_) return HB_OK;
    if (const int rc = idle()) return rc;
    release();
    const uint64_t want = need > grow_to ? need : grow_to;
    p_ = static_cast<T*>(Mem::alloc(static_cast<size_t>(want) * sizeof(T)));
    if (!p_) return HB_ENOMEM;
    cap_ = want;
    return HB_OK;
  }
  void release() {
    if (p_) Mem::free(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T* get() const { return p_; }
  uint64_t cap() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  uint64_t cap_ = 0;  // elements
};

}  // namespace hbmem

#endif  // HBMEM_H_
