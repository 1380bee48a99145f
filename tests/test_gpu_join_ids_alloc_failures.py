"""-m gpu: every allocation of freddy_gpu_knn_join_ids and freddy_gpu_ivpq_analogy fails once (the allocation seam, csrc/alloc_hook.h),
test_gpu_similarity_alloc_failures.py's frame: the call runs once on cold handles with the seam's counter read around it (A
allocations); then for every n in 1 .. A fresh handles are pinned, the n-th allocation from now fails, the call must return
FREDDY_E_NOMEM with a message and exactly one failed allocation, the handles must not be poisoned, and the same call made again must
return the oracle's lists."""
import numpy as np
import pytest

import approx_analogy_model as am
import ivpq_analogy_model as im
import join_ids_inputs as ji
import pv_model as pm
import util

pytestmark = pytest.mark.gpu

SHAPE = ji.SHAPES[0]
CASE = ji.CASES[1]          # more than one round at this shape: whatever a later round allocates is among the allocations


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    g.alloc_fail_nth(0)
    yield g
    g.alloc_fail_nth(0)


def _sweep(gpu, name, make, call, check, floor):
    handles = make()
    c0 = gpu.alloc_stats().calls
    check(call(*handles))
    A = gpu.alloc_stats().calls - c0
    for h in handles:
        h.close()
    assert A >= floor, f"{name}: the call made {A} allocations through the seam, the code allocates at least {floor}"
    for n in range(1, A + 1):
        what = f"{name} n={n}/{A}"
        handles = make()
        failed0 = gpu.alloc_stats().failed
        gpu.alloc_fail_nth(n)
        err = None
        try:
            call(*handles)
        except gpu.FreddyGpuError as e:
            err = e
        finally:
            gpu.alloc_fail_nth(0)
        assert err is not None, f"{what}: the call succeeded although one of its allocations was to fail"
        assert gpu.alloc_stats().failed - failed0 == 1, what
        assert err.code == gpu.E_NOMEM and gpu.load().freddy_gpu_last_error().decode().strip(), f"{what}: {err}"
        # not poisoned: a call that a healthy handle refuses for its arguments (k = 0) is refused for those, not with "unpin it"
        ivpq = handles[0]
        q, oi, od = np.zeros((1, ivpq.d), np.float32), np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)
        assert ivpq.lib.freddy_gpu_knn_join(ivpq.h, gpu._p(q), 1, 0, None, 0, 1, 1, 0, 1, 0.8, 10, gpu._p(oi), gpu._p(od), None) == -1, f"{what}: poisoned"
        check(call(*handles))
        for h in handles:
            h.close()
    print(f"alloc-failure sweep {name}: A = {A} allocations (floor {floor})")


# FLOORS, what every such call allocates on a cold handle: the join's nine workspaces of workspaces(), the pinned target block, the pinned
# row numbers and the landing zone = 12 (the traversal's buffers come on top); the analogy: the pinned block and the raw rows of the
# re-rank and the join's query block, then the join's other eight workspaces, its target block and its landing zone = 13
@pytest.mark.parametrize("own", [False, True])
def test_knn_join_ids(gpu, oracle, own):
    exp, eit = ji.expected(oracle, SHAPE, 1, CASE)
    assert eit > 1
    k, alpha, pvf, T, conf = CASE

    def make():
        return (gpu.IVPQIndex(*ji.pin_args(ji.tables(SHAPE))), gpu.VectorIndex(*ji.vec_table(SHAPE, "same")))

    def call(ivpq, vec):
        return ivpq.knn_join_ids(None if own else vec, ji.query_ids(), k, ji.targets(T), alpha, pvf, 1, confidence=conf)

    def check(res):
        gq, gi, gd, git = res
        assert np.array_equal(gq, ji.query_ids()) and git == eit
        util.assert_same_lists(gi, gd, exp, "knn_join_ids")

    _sweep(gpu, f"knn_join_ids own={own}", make, call, check, 12)


def test_ivpq_analogy(gpu, oracle):
    x, ids, t = ji.analogy_tables()
    triples = am.main_triples()[:40]
    tg, (alpha, pvf, conf) = ji.analogy_target_sets()["base300"]
    exp, stats, *_ = im.expected(oracle, oracle.ivpq_table(*ji.pin_args(t)), x, ids, triples, 1, 4, tg, alpha, pvf, 0, confidence=conf)

    def make():
        return (gpu.IVPQIndex(*ji.pin_args(t)), gpu.VectorIndex(ids, x))

    def call(ivpq, vec):
        return ivpq.analogy(vec, triples, 1, 4, target_ids=tg, alpha=alpha, pvf=pvf, method=0, confidence=conf), ivpq.last_approx_analogy_stats()

    def check(res):
        (gi, gs), st = res
        pm.same(gi, gs, exp, 1, "ivpq analogy")
        assert st == stats

    _sweep(gpu, "ivpq_analogy", make, call, check, 13)
