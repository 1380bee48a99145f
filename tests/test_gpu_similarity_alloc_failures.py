"""-m gpu: every allocation of freddy_gpu_similarity_pairs / _matrix / _join fails once (the allocation seam, csrc/alloc_hook.h),
test_gpu_alloc_failures.py's frame for calls that change no table: the call runs once on a cold handle with the seam's counter read
around it (A allocations, at least the FLOOR counted in csrc/similarity.hip); then for every n in 1 .. A a fresh handle is pinned, the n-th
allocation from now fails, the call must return FREDDY_E_NOMEM with a message and exactly one failed allocation, the handle must not
be poisoned, and the same call made again must answer as the model does."""
import ctypes as C

import numpy as np
import pytest

import similarity_inputs as si
import similarity_model as sm

pytestmark = pytest.mark.gpu

D, N = 25, 400


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    g.alloc_fail_nth(0)
    yield g
    g.alloc_fail_nth(0)


def _table():
    ids, x = si.table(D)
    return ids[:N], x[:N]


def _inputs():
    ids, x = _table()
    rng = np.random.default_rng(4)
    return si.draw_ids(ids, 33, rng), si.draw_ids(ids, 130, rng), si.draw_ids(ids, 130, rng)


def _same(got, exp):
    return len(got) == len(exp) and all(sm.same_floats(g, e) if np.asarray(e).dtype == np.float32 else np.array_equal(g, e) for g, e in zip(got, exp))


# FLOORS (similarity.hip): pairs -- the two id arrays, the values, the known bytes = 4;  matrix -- B ids, B rows, known_b, the A block, the
# result block = 5, + A's known bytes and the pinned row numbers when A is named by ids = 7;  join -- the matrix's, + counts and offsets,
# + the three arrays of matches when any are written
def _scenarios():
    ids, x = _table()
    a, b, c = _inputs()
    va = x[sm.rows_of(ids, ids[:20])]
    thr = si.join_threshold(*sm.matrix(ids, x, a, b), frac=0.2)
    return {
        "pairs": (lambda v: v.similarity_pairs(b, c), lambda: sm.pairs(ids, x, b, c), 4),
        "matrix by ids": (lambda v: v.similarity_matrix(a, b), lambda: sm.matrix(ids, x, a, b), 7),
        "matrix by vectors": (lambda v: v.similarity_matrix(va, b), lambda: sm.matrix(ids, x, va, b), 5),
        "join by ids": (lambda v: v.similarity_join(a, b, thr, max_pairs=10 ** 6), lambda: sm.join(ids, x, a, b, thr), 7 + 2 + 3),
        "join by vectors, counting": (lambda v: v.similarity_join(va, b, thr, max_pairs=0), lambda: sm.join(ids, x, va, b, thr, 0), 5 + 2),
    }


@pytest.mark.parametrize("name", ["pairs", "matrix by ids", "matrix by vectors", "join by ids", "join by vectors, counting"])
def test_every_allocation_fails_once(gpu, name):
    call, model, floor = _scenarios()[name]
    ids, x = _table()
    exp = model()
    vec = gpu.VectorIndex(ids, x)
    c0 = gpu.alloc_stats().calls
    got = call(vec)
    A = gpu.alloc_stats().calls - c0
    vec.close()
    assert _same(got, exp), f"{name}: the call differs from the model before anything fails"
    assert A >= floor, f"{name}: the call made {A} allocations through the seam, the code allocates at least {floor}"
    for n in range(1, A + 1):
        what = f"{name} n={n}/{A}"
        vec = gpu.VectorIndex(ids, x)
        failed0 = gpu.alloc_stats().failed
        gpu.alloc_fail_nth(n)
        err = None
        try:
            call(vec)
        except gpu.FreddyGpuError as e:
            err = e
        finally:
            gpu.alloc_fail_nth(0)
        assert err is not None, f"{what}: the call succeeded although one of its allocations was to fail"
        assert gpu.alloc_stats().failed - failed0 == 1, what
        assert err.code == gpu.E_NOMEM and gpu.load().freddy_gpu_last_error().decode().strip(), f"{what}: {err}"
        # not poisoned: a call that is refused for its arguments on a healthy handle (k = 0) is refused for those, not with "unpin it"
        oi, od, q = np.empty((1, 1), np.int32), np.empty((1, 1), np.float32), np.zeros((1, D), np.float32)
        assert vec.lib.freddy_gpu_exact_search(vec.h, gpu._p(q), 1, 0, None, 0, gpu._p(oi), gpu._p(od)) == -1, f"{what}: the handle is poisoned"
        assert _same(call(vec), exp), f"{what}: the call made again differs from the model"
        vec.close()
    print(f"alloc-failure sweep {name}: A = {A} allocations (floor {floor})")
