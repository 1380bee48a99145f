// alloc_hook.h -- the one seam every device / pinned-host allocation of the library goes through.  Plain C++17, no HIP: the real
// allocator and the real free are passed in as function pointers, so tests/test_alloc_hook_cpu.py compiles this file on its own
// with g++ over malloc / free.  internal.h wraps hipMalloc / hipFree / hipHostMalloc / hipHostFree around it; no other file of
// csrc calls those four.
//
// What it is for: the library lives in PostgreSQL backends that share a GPU, where a failed allocation is an ordinary event --
// and a failure branch that never ran is a branch nobody knows.  The seam lets a test say "the n-th allocation from now fails" and
// then look at what the call left behind:
//   a call counter      every allocation request, failed ones included (one relaxed atomic add: the default cost of the seam)
//   an armed countdown  the n-th allocation from now fails ONCE, then the seam is disarmed.  Injected (real = 0): the seam answers
//                       `oom` without calling the allocator.  Real (real != 0): the allocator is asked for kHugeRequest bytes, so
//                       that the failure -- and whatever state the runtime keeps about it -- is the runtime's own
//   tracking            off by default; on: a mutex-guarded map ptr -> bytes gives the live count, the live bytes and a 64-bit
//                       digest of the live set that does not depend on the order in which it came about
// Nothing here reads the environment: the three freddy_gpu_debug_alloc_* entry points (core.hip) are the only switches.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <unordered_map>

namespace freddy {
namespace alloc_hook {

constexpr size_t kHugeRequest = (size_t)1 << 60;   // what the real-failure mode asks the allocator for

struct Stats { int64_t calls, failed, live, live_bytes; uint64_t digest; };

struct State {
  std::atomic<int64_t> calls{0};
  std::atomic<int64_t> failed{0};      // allocations that returned an error: injected, forced through the allocator, or its own
  std::atomic<int64_t> countdown{0};   // > 0: armed -- the allocation that brings it to 0 fails
  std::atomic<int32_t> real{0};        // the armed failure comes from the allocator (kHugeRequest)
  std::atomic<int32_t> tracking{0};
  std::mutex mu;                       // guards live / live_bytes / digest
  std::unordered_map<const void*, size_t> live;
  int64_t live_bytes = 0;
  uint64_t digest = 0;
};
inline State& state() { static State s; return s; }

// splitmix64: one live entry's share of the digest.  The digest is the wrapping SUM of the shares, so it is a function of the
// live set alone; two different sets agree with probability ~2^-64.
inline uint64_t mix(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
inline uint64_t entry_digest(const void* p, size_t bytes) { return mix(mix((uint64_t)(uintptr_t)p) ^ (uint64_t)bytes); }

// The n-th allocation from now fails once (n <= 0: disarm).
inline void fail_nth(int64_t n, int32_t real) {
  State& st = state();
  st.real.store(real ? 1 : 0, std::memory_order_relaxed);
  st.countdown.store(n > 0 ? n : 0, std::memory_order_relaxed);
}
// Tracking on: from an empty map (what was allocated before is not known to it); off: the map is dropped.
inline void track(int32_t on) {
  State& st = state();
  std::lock_guard<std::mutex> g(st.mu);
  st.live.clear();
  st.live_bytes = 0;
  st.digest = 0;
  st.tracking.store(on ? 1 : 0, std::memory_order_relaxed);
}
inline Stats stats() {
  State& st = state();
  Stats s;
  s.calls = st.calls.load(std::memory_order_relaxed);
  s.failed = st.failed.load(std::memory_order_relaxed);
  std::lock_guard<std::mutex> g(st.mu);
  s.live = (int64_t)st.live.size();
  s.live_bytes = st.live_bytes;
  s.digest = st.digest;
  return s;
}

// 0: go on; 1: fail without the allocator; 2: fail through it
inline int armed_verdict(State& st) {
  int64_t c = st.countdown.load(std::memory_order_relaxed);
  while (c > 0) {
    if (st.countdown.compare_exchange_weak(c, c - 1, std::memory_order_relaxed))
      return c == 1 ? (st.real.load(std::memory_order_relaxed) ? 2 : 1) : 0;
  }
  return 0;
}

// One allocation: real_alloc(out, bytes) returns `ok` on success.  An injected failure returns `oom` and leaves *out NULL.
template <class Err, class Alloc>
inline Err allocate(Alloc real_alloc, void** out, size_t bytes, Err ok, Err oom) {
  State& st = state();
  st.calls.fetch_add(1, std::memory_order_relaxed);
  if (st.countdown.load(std::memory_order_relaxed) > 0) {
    const int v = armed_verdict(st);
    if (v == 1) {
      *out = nullptr;
      st.failed.fetch_add(1, std::memory_order_relaxed);
      return oom;
    }
    if (v == 2) bytes = kHugeRequest;
  }
  const Err e = real_alloc(out, bytes);
  if (e != ok) {
    *out = nullptr;
    st.failed.fetch_add(1, std::memory_order_relaxed);
    return e;
  }
  if (st.tracking.load(std::memory_order_relaxed)) {
    std::lock_guard<std::mutex> g(st.mu);
    if (st.tracking.load(std::memory_order_relaxed) && st.live.emplace(*out, bytes).second) {
      st.live_bytes += (int64_t)bytes;
      st.digest += entry_digest(*out, bytes);
    }
  }
  return e;
}

// One free.  The entry leaves the map before the memory goes back, so that another thread's allocation of the same address finds
// its place free.
template <class Free>
inline auto release(Free real_free, void* p) -> decltype(real_free(p)) {
  State& st = state();
  if (p && st.tracking.load(std::memory_order_relaxed)) {
    std::lock_guard<std::mutex> g(st.mu);
    auto it = st.live.find(p);
    if (it != st.live.end()) {
      st.live_bytes -= (int64_t)it->second;
      st.digest -= entry_digest(p, it->second);
      st.live.erase(it);
    }
  }
  return real_free(p);
}

}  // namespace alloc_hook
}  // namespace freddy
