// Owners of what the C ABI's host side holds on the device: DevBuf<T> (device memory), PinBuf<T> (pinned host memory) and
// Event (a hipEventDisableTiming event).  Move-only; each releases what it holds in its destructor, so the structs of
// si_internal.h free a context's memory by being destroyed or assigned a fresh value, not by hand-written lists.
// Device memory is reached through exactly two functions, defined once in capi.hip: that definition is the one place where
// the development build switches to the guard-page allocator (guard_alloc.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace si {

hipError_t raw_dev_malloc(void** out, size_t bytes);
hipError_t raw_dev_free(void* p);

namespace detail {
struct DevMem {
  static hipError_t get(void** out, size_t bytes) { return raw_dev_malloc(out, bytes); }
  static void put(void* p) { (void)raw_dev_free(p); }
};
struct PinMem {
  static hipError_t get(void** out, size_t bytes) { return hipHostMalloc(out, bytes, hipHostMallocDefault); }
  static void put(void* p) { (void)hipHostFree(p); }
};

// A pointer plus its element count.  Converts implicitly to T*, so `buf + off`, `buf[i]`, `!buf` and passing it where a
// kernel launcher takes a pointer all read as they would on the raw pointer.
template <typename T, typename Mem>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t size() const { return n_; }   // elements; 0 when empty

  // drops the old buffer, THEN allocates `count` elements (one when count == 0); the owner is empty when that fails
  hipError_t try_alloc(size_t count) {   // (for the callers that report the runtime's own error)
    reset();
    if (count == 0) count = 1;
    void* q = nullptr;
    const hipError_t e = Mem::get(&q, count * sizeof(T));
    if (e != hipSuccess || !q) return e != hipSuccess ? e : hipErrorOutOfMemory;
    p_ = static_cast<T*>(q), n_ = count;
    return hipSuccess;
  }
  bool alloc(size_t count) { return try_alloc(count) == hipSuccess; }
  // grow on demand: nothing happens while size() >= count; else as alloc (the old buffer goes first: both at once would
  // raise the memory peak of the largest constructions).  An empty owner has size() 0 and always allocates.
  bool reserve(size_t count) { return (p_ && n_ >= count) || alloc(count); }
  void reset() {
    if (p_) Mem::put(p_);
    p_ = nullptr, n_ = 0;
  }
  // hand-over of a buffer allocated elsewhere / to elsewhere
  void adopt(T* p, size_t count) {
    reset();
    p_ = p, n_ = p ? count : 0;
  }
  T* release() {
    T* p = p_;
    p_ = nullptr, n_ = 0;
    return p;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
}  // namespace detail

template <typename T>
using DevBuf = detail::Buf<T, detail::DevMem>;
template <typename T>
using PinBuf = detail::Buf<T, detail::PinMem>;

class Event {
 public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) {
      reset();
      e_ = o.e_;
      o.e_ = nullptr;
    }
    return *this;
  }
  ~Event() { reset(); }

  operator hipEvent_t() const { return e_; }
  hipError_t try_create() {   // (a second create replaces the event)
    reset();
    return hipEventCreateWithFlags(&e_, hipEventDisableTiming);
  }
  bool create() { return try_create() == hipSuccess; }
  void reset() {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace si
