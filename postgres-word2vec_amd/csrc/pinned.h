// pinned.h -- page-locked host memory that the kernels read and write themselves (mapped into the device's address space):
// the staging buffers of the host-buffer calls, and the bounded wait on a word a kernel writes there last.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_alloc.h"

#include <atomic>
#include <chrono>
#include <cstring>

// The host-memory counterpart of DevBuf: grown on demand (contents are not kept), with a quarter of headroom.
struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    release();
    const size_t want = bytes + bytes / 4 + 256;
    if (host_malloc(&p, want) != hipSuccess) { p = nullptr; return -1; }
    cap = want;
    return 0;
  }
  void release() { if (p) (void)host_free(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// the device-side address of a pinned (PinnedBuf / freddy_gpu_host_alloc) host buffer, or NULL for ordinary memory
static inline const void* pinned_device_pointer(const void* p) {
  hipPointerAttribute_t attr;
  memset(&attr, 0, sizeof(attr));
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return attr.type == hipMemoryTypeHost ? attr.devicePointer : nullptr;
}

// Spin on a word of mapped host memory until a kernel has set it (non-zero) or `us` microseconds have passed -- a few
// microseconds sooner than the runtime's completion signal -- then order the reads behind it.  Returns the word: 0 = not
// yet, the caller waits for its stream or event the usual way.
static inline int32_t wait_word(volatile const int32_t* w, int us) {
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(us);
  int spins = 0;
  while (*w == 0) {
    __builtin_ia32_pause();
    if ((++spins & 255) == 0 && std::chrono::steady_clock::now() > t_end) break;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return *w;
}
