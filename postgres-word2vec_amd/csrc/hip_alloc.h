// hip_alloc.h -- the HIP side of the allocation seam (alloc_hook.h: counter, injected failures, tracking): the four wrappers that
// are the ONLY callers of hipMalloc / hipFree / hipHostMalloc / hipHostFree in csrc.  A header of its own, below internal.h, because
// pinned.h and join_index.h allocate too and are compiled without internal.h (tests/test_codegen.py builds kernels from their headers).
#pragma once
#include <hip/hip_runtime.h>

// Every device / pinned-host allocation and free of the library goes through these (tests/test_alloc_hook_cpu.py reads csrc and
// fails on a raw call anywhere else).  A failed allocation is an ordinary event beside other backends: the runtime's sticky
// last-error word is cleared HERE, so that the hipGetLastError() behind the next launch reports that launch and not this failure.
#include "alloc_hook.h"
template <class T>
static inline hipError_t dev_malloc(T** out, size_t bytes) {
  const hipError_t e = freddy::alloc_hook::allocate(+[](void** p, size_t n) { return hipMalloc(p, n); }, (void**)out, bytes, hipSuccess, hipErrorOutOfMemory);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}
static inline hipError_t dev_free(void* p) { return freddy::alloc_hook::release(+[](void* q) { return hipFree(q); }, p); }
static inline hipError_t host_malloc(void** out, size_t bytes) {
  const hipError_t e = freddy::alloc_hook::allocate(+[](void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }, out, bytes, hipSuccess, hipErrorOutOfMemory);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}
static inline hipError_t host_free(void* p) { return freddy::alloc_hook::release(+[](void* q) { return hipHostFree(q); }, p); }
