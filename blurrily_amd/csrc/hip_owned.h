// hip_owned.h -- what the host code holds of the HIP runtime, each in an owner that gives it back when it goes: a stream,
// a set of events, a pinned host page, a device allocation.  All are move-only; an owner of nothing makes no HIP call,
// so an object full of them that never met a GPU is made and dropped without one.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>

#include "hip_try.h"

namespace blurrily {
namespace detail __attribute__((visibility("hidden"))) {

// One handle or pointer H, given back by Release()(h).  It reads as the handle wherever one is expected.
template <class H, class Release>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Owned& operator=(Owned&& o) noexcept { if (this != &o) reset(std::exchange(o.h, nullptr)); return *this; }
  ~Owned() { reset(); }
  void reset(H next = nullptr) { if (h) Release()(h); h = next; }
  operator H() const { return h; }
};
struct StreamRelease { void operator()(hipStream_t s) const { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } };
struct EventRelease  { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct HostRelease   { void operator()(void* p) const { (void)hipHostFree(p); } };
struct DeviceRelease { void operator()(void* p) const { (void)hipFree(p); } };

// A non-blocking stream (the only kind made here), synchronised before it is destroyed.
struct Stream : Owned<hipStream_t, StreamRelease> {
  int make() {                                            // (made already: nothing to do)
    if (h) return 0;
    BLURRILY_HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
    return 0;
  }
};

// N events with the same flags, all of them or none: a half-made set would be recorded into.
template <int N>
struct Events {
  Owned<hipEvent_t, EventRelease> e[N];
  explicit operator bool() const { return e[0] != nullptr; }
  hipEvent_t operator[](int i) const { return e[i]; }
  int make(unsigned flags = hipEventDefault) {            // (made already: nothing to do)
    if (*this) return 0;
    Events made;
    for (auto& x : made.e) BLURRILY_HIP_TRY(hipEventCreateWithFlags(&x.h, flags));
    *this = std::move(made);
    return 0;
  }
};

// Pinned host memory (flags: hipHostMallocDefault, or mapped and coherent where the device reads and writes it in place).
struct HostPage : Owned<unsigned char*, HostRelease> {
  int alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
    reset();
    BLURRILY_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h), bytes, flags));
    return 0;
  }
};

// n objects of T in device memory, made once and kept.
template <class T>
struct DeviceMem : Owned<T*, DeviceRelease> {
  int alloc(size_t n) {
    if (this->h) return 0;
    BLURRILY_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&this->h), n * sizeof(T)));
    return 0;
  }
};

// Device scratch that only ever grows.
struct DeviceBuffer {
  void*  p = nullptr;
  size_t bytes = 0;
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) { release(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); }
    return *this;
  }
  ~DeviceBuffer() { release(); }
  int reserve(size_t want, hipStream_t stream) {
    if (want <= bytes) return 0;
    if (p) { (void)hipStreamSynchronize(stream); release(); }
    const size_t grow = std::max(want, bytes + bytes / 2);
    BLURRILY_HIP_TRY(hipMalloc(&p, grow));
    bytes = grow;
    return 0;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

template <class T> constexpr bool kMoveOnly = std::is_move_constructible<T>::value && std::is_move_assignable<T>::value &&
                                              !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value;
static_assert(kMoveOnly<Stream>, "a stream has one owner");
static_assert(kMoveOnly<Events<2>>, "a set of events has one owner");
static_assert(kMoveOnly<HostPage>, "a pinned page has one owner");
static_assert(kMoveOnly<DeviceMem<unsigned>>, "a device allocation has one owner");
static_assert(kMoveOnly<DeviceBuffer>, "device scratch has one owner");

}  // namespace detail
}  // namespace blurrily
