// Owning types for what the library takes from the HIP runtime: device memory, page-locked host memory, events and
// streams.  All are move-only, empty when default-constructed, and release what they hold in their destructor -- a
// resource of the context (vcy_ctx) is a member of one of these types, a temporary of a function a local of one, and
// nothing is freed by name.  Every operation answers with the runtime's own error code; callers check it.
// Next to them PoolLayout, which places the arrays of one pooled buffer.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace vcy {

struct DeviceMemory {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t release(void* p) { return hipFree(p); }  // (waits for the device)
};
template <unsigned Flags>
struct PinnedMemory {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
  static hipError_t release(void* p) { return hipHostFree(p); }
};

// Pointer and capacity of one allocation.  Reads as a T* wherever one is expected (`c->d_sdf + n`, kernel arguments,
// `if (!c->d_cnt)`), and casts like one (`(char*)c->d_cnt`).
template <class T, class Memory>
class Buffer {
 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { (void)reset(); }

  operator T*() const { return (T*)p_; }
  template <class U>
  explicit operator U*() const { return (U*)p_; }
  size_t bytes() const { return bytes_; }

  // Empty afterwards, whatever the runtime answers.
  hipError_t reset() {
    void* old = std::exchange(p_, nullptr);
    bytes_ = 0;
    return old ? Memory::release(old) : hipSuccess;
  }
  // `bytes` newly allocated in place of what was held; empty after a failure (best-effort callers clear the error and
  // go on without the buffer).
  hipError_t alloc(size_t bytes) {
    hipError_t e = reset();
    if (e == hipSuccess) e = Memory::alloc(&p_, bytes);
    if (e == hipSuccess) bytes_ = bytes;
    else p_ = nullptr;
    return e;
  }
  // Grow-only: at least `want` bytes, no headroom (a caller that wants some asks for it).  Before the old buffer is freed
  // the work on `wait_for` is waited for, unless the caller knows that nothing in flight uses it (`wait` false).
  hipError_t grow(size_t want, hipStream_t wait_for, bool wait = true) {
    if (bytes_ >= want) return hipSuccess;
    const hipError_t e = wait ? hipStreamSynchronize(wait_for) : hipSuccess;
    return e == hipSuccess ? alloc(want) : e;
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

template <class T = void>
using DeviceBuf = Buffer<T, DeviceMemory>;
template <class T = void, unsigned Flags = hipHostMallocDefault>
using PinnedBuf = Buffer<T, PinnedMemory<Flags>>;

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The arrays of one pooled buffer (a grow-only DeviceBuf of the context), one behind the other in the order they are
// taken, each at a multiple of 256 bytes: `take` answers an array's offset, `total` the bytes the buffer must hold.
class PoolLayout {
 public:
  size_t take(size_t bytes) { return std::exchange(at_, at_ + align256(bytes)); }
  size_t total() const { return at_; }

 private:
  size_t at_ = 0;
};

// An event, created on first use.
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept {
    std::swap(e_, o.e_);
    return *this;
  }
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  hipError_t ensure(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

// A stream the context created, or one it was handed (vcy_set_stream) and does not own.
class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { (void)release(); }
  hipError_t create(unsigned flags) {
    hipError_t e = release();
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s_, flags);
    owned_ = e == hipSuccess;
    return e;
  }
  void borrow(hipStream_t s) {  // (after release())
    s_ = s;
    owned_ = false;
  }
  hipError_t release() {
    hipStream_t old = std::exchange(s_, nullptr);
    return std::exchange(owned_, false) && old ? hipStreamDestroy(old) : hipSuccess;
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
  bool owned_ = false;
};

}  // namespace vcy
