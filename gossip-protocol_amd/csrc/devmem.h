// devmem.h — move-only owners of device memory, pinned host memory and events.
//
// Thin wrappers over hipMalloc / hipFree, hipHostMalloc / hipHostFree and hipEventCreate /
// hipEventDestroy: no pooling, no registry, no policy.  An owner frees what it holds when it
// goes out of scope; it converts to the raw pointer (or event), so kernel-argument structs and
// launch wrappers keep taking plain pointers as views.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace gossip {

namespace detail {
struct DeviceMem {
  static hipError_t get(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
  static hipError_t put(void* p) { return hipFree(p); }
};
struct PinnedMem {
  static hipError_t get(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
  static hipError_t put(void* p) { return hipHostFree(p); }
};

// `count` elements of T from Mem, freed on destruction
template <class T, class Mem>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      (void)reset();
      swap(o);
    }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { (void)reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t count() const { return n_; }
  void swap(Owned& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(n_, o.n_);
  }
  // Frees; the owner is empty afterwards whatever the free returned.
  hipError_t reset() {
    T* p = std::exchange(p_, nullptr);
    n_ = 0;
    return p ? Mem::put(p) : hipSuccess;
  }

 protected:
  hipError_t take(size_t count, unsigned flags) {
    (void)reset();
    void* p = nullptr;
    const hipError_t rc = Mem::get(&p, count * sizeof(T), flags);
    if (rc != hipSuccess) {
      (void)hipGetLastError();  // reported here: the next launch's error check must not find it
      return rc;
    }
    p_ = (T*)p;
    n_ = count;
    return hipSuccess;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
}  // namespace detail

// Device buffer of `count` T.  Byte slabs that are carved into several arrays are DevBuf<uint8_t>.
template <class T>
class DevBuf : public detail::Owned<T, detail::DeviceMem> {
 public:
  // A fresh allocation (what was held is freed first).  zero: hipMemset on the null stream, which
  // a non-blocking stream does not wait for; a failed memset leaves the buffer held.
  hipError_t alloc(size_t count, bool zero) {
    if (hipError_t rc = this->take(count, 0)) return rc;
    return zero ? hipMemset(this->get(), 0, count * sizeof(T)) : hipSuccess;
  }
  // Room for `count` elements: kept when it is there, else the old buffer is freed (hipFree waits
  // for the device) before count + slack elements are allocated; the contents are not carried over.
  hipError_t reserve(size_t count, size_t slack) {
    if (this->get() && count <= this->count()) return hipSuccess;
    if (hipError_t rc = this->reset()) return rc;
    return alloc(count + slack, false);
  }
};

// Pinned host buffer of `count` T (flags: hipHostMallocDefault, hipHostMallocMapped, ...).
template <class T>
class PinBuf : public detail::Owned<T, detail::PinnedMem> {
 public:
  hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) { return this->take(count, flags); }
};

class DevEvent {
 public:
  DevEvent() = default;
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
  ~DevEvent() {
    if (ev_) (void)hipEventDestroy(ev_);
  }
  hipError_t create() { return ev_ ? hipSuccess : hipEventCreate(&ev_); }
  operator hipEvent_t() const { return ev_; }

 private:
  hipEvent_t ev_ = nullptr;
};

}  // namespace gossip
