"""-m gpu: every allocation of freddy_gpu_tokenize and of freddy_gpu_exact_search_texts fails once (the allocation seam,
csrc/alloc_hook.h), test_gpu_join_ids_alloc_failures.py's frame: the call runs once on a cold handle with the seam's counter read
around it (A allocations); then for every n in 1 .. A a fresh handle is pinned, the n-th allocation from now fails, the call must
return FREDDY_E_NOMEM with a message and exactly one failed allocation, the handle's bytes (freddy_gpu_index_bytes) are what they
were, it is not poisoned, and the same call made again answers as the model does."""
import numpy as np
import pytest

import tokenize_inputs as ti
import tokenize_model as tm

pytestmark = pytest.mark.gpu
U = np.uint32
D = 64


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    g.alloc_fail_nth(0)
    yield g
    g.alloc_fail_nth(0)


@pytest.fixture(scope="module")
def case(gpu, oracle):
    ids, v = ti.table(D)
    texts = [x for _, x in ti.texts(ids) if len(x) <= 257]
    exp = tm.tokenize(oracle, ids, v, texts, tm.TABLE_ORDER, True)
    ref = gpu.VectorIndex(ids, v)
    live = exp[1] > 0
    lists = ref.search(np.ascontiguousarray(exp[0][live]), 5)
    ref.close()
    return {"ids": ids, "v": v, "texts": texts, "exp": exp, "live": live, "lists": lists}


def _sweep(gpu, name, make, call, check, floor):
    h = make()
    c0 = gpu.alloc_stats().calls
    check(call(h))
    A = gpu.alloc_stats().calls - c0
    h.close()
    assert A >= floor, f"{name}: the call made {A} allocations through the seam, the code allocates at least {floor}"
    for n in range(1, A + 1):
        what = f"{name} n={n}/{A}"
        h = make()
        bytes0, failed0 = h.nbytes, gpu.alloc_stats().failed
        gpu.alloc_fail_nth(n)
        err = None
        try:
            call(h)
        except gpu.FreddyGpuError as e:
            err = e
        finally:
            gpu.alloc_fail_nth(0)
        assert err is not None, f"{what}: the call succeeded although one of its allocations was to fail"
        assert gpu.alloc_stats().failed - failed0 == 1, what
        assert err.code == gpu.E_NOMEM and gpu.load().freddy_gpu_last_error().decode().strip(), f"{what}: {err}"
        assert h.nbytes == bytes0, what
        # not poisoned: a call that a healthy handle refuses for its arguments (k = 0) is refused for those, not with "unpin it"
        q, oi, od = np.zeros((1, D), np.float32), np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)
        assert h.lib.freddy_gpu_exact_search(h.h, gpu._p(q), 1, 0, None, 0, gpu._p(oi), gpu._p(od)) == -1, f"{what}: poisoned"
        check(call(h))
        h.close()
    print(f"alloc-failure sweep {name}: A = {A} allocations (floor {floor})")


# FLOORS, what the calls allocate on a cold handle.  tokenize: the vectors, the centroids in front of the normalisation, the texts
# on the device = 3.  exact_search_texts: the texts on the device, the pinned block of a pass, the centroids = 3, then what
# freddy_gpu_exact_search allocates for the pass (the queries, the two result arrays and the partial lists at least) = 7.
def test_tokenize(gpu, case):
    def check(res):
        gv, gc = res
        assert np.array_equal(gc, case["exp"][1]) and np.array_equal(gv.view(U), case["exp"][0].view(U))

    _sweep(gpu, "tokenize", lambda: gpu.VectorIndex(case["ids"], case["v"]), lambda h: h.tokenize(case["texts"]), check, 3)


def test_exact_search_texts(gpu, case):
    live = case["live"]

    def check(res):
        gc, gi, gs = res
        assert np.array_equal(gc, case["exp"][1])
        assert np.array_equal(gi[live], case["lists"][0]) and np.array_equal(gs[live].view(U), case["lists"][1].view(U))
        assert (gi[~live] == -1).all() and np.isneginf(gs[~live]).all()

    _sweep(gpu, "exact_search_texts", lambda: gpu.VectorIndex(case["ids"], case["v"]), lambda h: h.search_texts(case["texts"], 5), check, 7)
