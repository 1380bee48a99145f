"""The allocation seam (postgres-word2vec_amd/csrc/alloc_hook.h) on its own, and the rule that nothing in csrc goes round it.

alloc_hook.h is plain C++ (no HIP): compiled here with g++ behind a small C wrapper whose "runtime" is malloc / free, as
test_registry.py does for the registry.  Properties: the n-th failure fires exactly once and the calls around it succeed; the
counters are exact; the digest of the live set is a function of the set alone (equal sets built in different orders agree,
different sets differ); eight threads lose no count.  The GPU tests (test_gpu_alloc_failures*.py) then rely on the seam to visit
every failure branch of the library -- which they can only do if every allocation goes through it: the last test reads csrc and
fails on a raw call outside the wrappers."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")

WRAPPER = r"""
#include <stdlib.h>
#include <thread>
#include <vector>
#include "alloc_hook.h"
namespace ah = freddy::alloc_hook;
// the stand-in runtime: 0 = success, 2 = out of memory; a request of kHugeRequest bytes fails as a real one would
static int real_alloc(void** p, size_t n) {
  if (n >= ah::kHugeRequest) { *p = nullptr; return 2; }
  *p = malloc(n ? n : 1);
  return *p ? 0 : 2;
}
static int real_free(void* p) { free(p); return 0; }
static long long g_real_calls = 0;   // calls that reached the stand-in runtime (single-threaded tests only)
static int counted_alloc(void** p, size_t n) { ++g_real_calls; return real_alloc(p, n); }
extern "C" {
int ah_alloc(void** out, size_t n) { return ah::allocate(&counted_alloc, out, n, 0, 2); }
int ah_free(void* p) { return ah::release(&real_free, p); }
long long ah_real_calls() { return g_real_calls; }
void ah_fail_nth(long long n, int real) { ah::fail_nth(n, real); }
void ah_track(int on) { ah::track(on); }
void ah_stats(long long* out5) {
  const ah::Stats s = ah::stats();
  out5[0] = s.calls; out5[1] = s.failed; out5[2] = s.live; out5[3] = s.live_bytes; out5[4] = (long long)s.digest;
}
// n_threads threads, each `rounds` times: allocate `per` blocks, free them.  Returns the failures the threads saw.
long long ah_hammer(int n_threads, int rounds, int per) {
  std::vector<long long> failed((size_t)n_threads, 0);
  std::vector<std::thread> th;
  for (int t = 0; t < n_threads; ++t)
    th.emplace_back([&, t] {
      std::vector<void*> held((size_t)per);
      for (int r = 0; r < rounds; ++r) {
        for (int i = 0; i < per; ++i) if (ah::allocate(&real_alloc, &held[(size_t)i], (size_t)(16 + 8 * i + t), 0, 2) != 0) { ++failed[(size_t)t]; held[(size_t)i] = nullptr; }
        for (int i = 0; i < per; ++i) if (held[(size_t)i]) ah::release(&real_free, held[(size_t)i]);
      }
    });
  for (auto& x : th) x.join();
  long long sum = 0;
  for (long long f : failed) sum += f;
  return sum;
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not on PATH")
    d = tmp_path_factory.mktemp("alloc_hook")
    src = d / "wrap.cpp"
    src.write_text(WRAPPER)
    so = d / "libah.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, str(src), "-o", str(so), "-pthread"], check=True)
    lib = ctypes.CDLL(str(so))
    lib.ah_alloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.ah_free.argtypes = [ctypes.c_void_p]
    lib.ah_fail_nth.argtypes = [ctypes.c_longlong, ctypes.c_int]
    lib.ah_real_calls.restype = ctypes.c_longlong
    lib.ah_hammer.restype = ctypes.c_longlong
    return lib


def _stats(lib):
    out = (ctypes.c_longlong * 5)()
    lib.ah_stats(out)
    return dict(calls=out[0], failed=out[1], live=out[2], live_bytes=out[3], digest=out[4] & (2 ** 64 - 1))


def _alloc(lib, n):
    p = ctypes.c_void_p()
    rc = lib.ah_alloc(ctypes.byref(p), n)
    return rc, p.value


@pytest.fixture()
def clean(lib):
    lib.ah_fail_nth(0, 0)
    lib.ah_track(0)
    yield lib
    lib.ah_fail_nth(0, 0)
    lib.ah_track(0)


@pytest.mark.parametrize("n", [1, 2, 7])
def test_nth_failure_fires_exactly_once(clean, n):
    """armed with n: allocations 1 .. n-1 succeed, the n-th fails WITHOUT reaching the runtime and leaves NULL, and every later one
    succeeds (the seam has disarmed itself)."""
    lib = clean
    before, real_before = _stats(lib), lib.ah_real_calls()
    lib.ah_fail_nth(n, 0)
    held, verdicts = [], []
    for i in range(1, n + 6):
        rc, p = _alloc(lib, 100 + i)
        verdicts.append(rc)
        if rc == 0:
            assert p
            held.append(p)
        else:
            assert rc == 2 and p is None
    assert verdicts == [0] * (n - 1) + [2] + [0] * 5
    after = _stats(lib)
    assert after["calls"] - before["calls"] == n + 5          # the failed call counts as a call
    assert after["failed"] - before["failed"] == 1
    assert lib.ah_real_calls() - real_before == n + 4        # the injected failure never reached the runtime
    for p in held:
        assert lib.ah_free(p) == 0


def test_real_mode_fails_through_the_runtime_once(clean):
    """real != 0: the armed allocation is forwarded with the huge request, so the failure is the runtime's own; once."""
    lib = clean
    before, real_before = _stats(lib), lib.ah_real_calls()
    lib.ah_fail_nth(2, 1)
    rcs = []
    for _ in range(4):
        rc, p = _alloc(lib, 64)
        rcs.append(rc)
        if p:
            lib.ah_free(p)
    assert rcs == [0, 2, 0, 0]
    assert lib.ah_real_calls() - real_before == 4               # all four reached the runtime
    assert _stats(lib)["failed"] - before["failed"] == 1


def test_disarm_and_rearm(clean):
    lib = clean
    lib.ah_fail_nth(1, 0)
    lib.ah_fail_nth(0, 0)                                      # disarmed before it fired
    rc, p = _alloc(lib, 8)
    assert rc == 0
    lib.ah_free(p)
    lib.ah_fail_nth(3, 0)
    lib.ah_fail_nth(1, 0)                                      # re-armed: the later order holds
    assert _alloc(lib, 8)[0] == 2
    rc, p = _alloc(lib, 8)
    assert rc == 0
    lib.ah_free(p)


def test_tracking_counts_live_blocks_and_bytes(clean):
    lib = clean
    rc, untracked = _alloc(lib, 1000)                          # before tracking: unknown to the map, also when it is freed later
    assert rc == 0
    lib.ah_track(1)
    assert _stats(lib)["live"] == 0 and _stats(lib)["live_bytes"] == 0 and _stats(lib)["digest"] == 0
    sizes = [1, 17, 4096, 300]
    ptrs = [_alloc(lib, s)[1] for s in sizes]
    st = _stats(lib)
    assert st["live"] == 4 and st["live_bytes"] == sum(sizes) and st["digest"] != 0
    lib.ah_free(untracked)
    assert _stats(lib)["live"] == 4 and _stats(lib)["live_bytes"] == sum(sizes)
    lib.ah_fail_nth(1, 0)
    assert _alloc(lib, 50)[0] == 2                             # a failed allocation is not live
    assert _stats(lib)["live"] == 4
    lib.ah_free(ptrs.pop(1))
    st = _stats(lib)
    assert st["live"] == 3 and st["live_bytes"] == sum(sizes) - 17
    lib.ah_free(None)                                          # free(NULL): no entry, no change
    assert _stats(lib)["live"] == 3
    for p in ptrs:
        lib.ah_free(p)
    st = _stats(lib)
    assert st["live"] == 0 and st["live_bytes"] == 0 and st["digest"] == 0
    lib.ah_track(0)
    rc, p = _alloc(lib, 9)
    assert _stats(lib)["live"] == 0                            # off: nothing is recorded
    lib.ah_free(p)


def test_digest_is_a_function_of_the_live_set(clean):
    """1000 random alloc / free sequences, each built two ways.  The digest after each equals a Python model of the live set
    {(address, bytes)} -- so it does not depend on the order -- and the same set reached by a different order of the same frees
    gives the same digest, while freeing one more block (a different set) changes it."""
    lib = clean
    M = 2 ** 64 - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    def model(live):
        return sum(mix(mix(p) ^ n) for p, n in live.items()) & M

    rng = random.Random(1234)
    lib.ah_track(1)
    seen = {}
    for _ in range(1000):
        live = {}
        for _ in range(rng.randint(1, 12)):
            n = rng.choice([1, 8, 24, 100, 513, 4096])
            rc, p = _alloc(lib, n)
            assert rc == 0
            live[p] = n
        doomed = rng.sample(sorted(live), rng.randint(0, len(live) - 1))
        # way one: free in the sampled order; way two: free the same blocks in reverse AFTER allocating and freeing a bystander
        half = len(doomed) // 2
        for p in doomed[:half]:
            lib.ah_free(p)
            del live[p]
        assert _stats(lib)["digest"] == model(live)
        rc, by = _alloc(lib, 77)
        assert _stats(lib)["digest"] == model({**live, by: 77}) != model(live)      # a different set: a different digest
        lib.ah_free(by)
        for p in reversed(doomed[half:]):
            lib.ah_free(p)
            del live[p]
        st = _stats(lib)
        assert st["digest"] == model(live) and st["live"] == len(live) and st["live_bytes"] == sum(live.values())
        key = frozenset(live.items())
        assert seen.setdefault(key, st["digest"]) == st["digest"]                    # equal sets agree ...
        for p in list(live):
            lib.ah_free(p)
        assert _stats(lib)["digest"] == 0
        seen[frozenset()] = 0
    digests = {}
    for key, dg in seen.items():                                                     # ... and only equal sets do
        assert digests.setdefault(dg, key) == key


def test_eight_threads_lose_no_count(clean):
    """8 threads x 200 rounds x 16 blocks: every call is counted, the one armed failure fires in exactly one thread, and with
    tracking on nothing is left live."""
    lib = clean
    lib.ah_track(1)
    before = _stats(lib)
    lib.ah_fail_nth(5000, 0)
    failures = lib.ah_hammer(8, 200, 16)
    after = _stats(lib)
    assert after["calls"] - before["calls"] == 8 * 200 * 16
    assert failures == 1 and after["failed"] - before["failed"] == 1
    assert after["live"] == 0 and after["live_bytes"] == 0 and after["digest"] == 0
    assert _alloc(lib, 8)[0] == 0                                # disarmed (the block is dropped with the map)


RAW = re.compile(r"\bhip(Malloc|Free|HostMalloc|HostFree|MallocAsync|FreeAsync|MallocManaged|ExtMallocWithFlags|MallocPitch|HostAlloc|MallocHost|FreeHost)\s*\(")


def _code_only(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return "\n".join(re.sub(r"//.*", "", line) for line in text.split("\n"))


def test_no_raw_allocation_outside_the_wrappers():
    """Every device / pinned-host allocation and free of csrc goes through dev_malloc / dev_free / host_malloc / host_free
    (hip_alloc.h, which internal.h includes): a raw runtime call anywhere else would be an allocation the sweeps cannot fail and the tracker cannot see.  The
    four wrappers themselves hold exactly one raw call each."""
    raw = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".h", ".hip", ".inc", ".cpp")):
            continue
        code = _code_only(open(os.path.join(CSRC, f)).read())
        hits = [(i + 1, m.group(0)) for i, line in enumerate(code.split("\n")) for m in RAW.finditer(line)]
        if hits:
            raw[f] = hits
    assert set(raw) == {"hip_alloc.h"}, {f: h for f, h in raw.items() if f != "hip_alloc.h"}
    assert sorted(h[1].rstrip("(").strip() for h in raw["hip_alloc.h"]) == ["hipFree", "hipHostFree", "hipHostMalloc", "hipMalloc"], raw["hip_alloc.h"]
    internal = _code_only(open(os.path.join(CSRC, "hip_alloc.h")).read())
    for wrapper, call in (("dev_malloc", "hipMalloc"), ("dev_free", "hipFree"), ("host_malloc", "hipHostMalloc"), ("host_free", "hipHostFree")):
        body = re.search(r"static inline hipError_t %s\([^)]*\)\s*\{(.*?)\n\}|static inline hipError_t %s\([^)]*\)\s*\{(.*?)\}\n" % (wrapper, wrapper), internal, re.S)
        assert body, wrapper
        text = body.group(1) or body.group(2)
        assert "alloc_hook::" in text and re.search(r"\b%s\s*\(" % call, text), wrapper
    hook = open(os.path.join(CSRC, "alloc_hook.h")).read()
    assert "#include <hip" not in hook and "getenv" not in _code_only(hook)          # plain C++, and nothing reads the environment
