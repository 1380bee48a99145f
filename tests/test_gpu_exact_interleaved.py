"""-m gpu: exact kNN, the exact join and the exact analogies taking turns on ONE vector handle.  kNN and the join enqueue their
filter + refine chain through one host function and keep its state on the handle (the words in exf_small, the query fragments,
the sample, the candidate buffers, the self-check counters, the flag that says the words must be cleared); the analogies size
and overwrite the same buffers.  Every call's lists must be bit for bit those of the same call on a handle of its own and those
of the oracle / the numpy model, and the profile must show that the filter answered it, not the all-exact kernels.

The smallest shapes that reach every branch: a table of 2 080 x 32 (65 strips: the threshold comes from a sample), 70 queries
(two kNN tiles of 64, the second with 6 queries in one 32-query fragment tile), a join of the 70 over 100 target rows (one pass, a
last strip of 4 rows; 70 queries take the 128-query tile, so the last join asks for tiles of 64: two fragment tiles), 40 triples
(a pass of 32 and one of 8).  The sequence runs again with check_brackets bits 2 and 3: every buffer sized to refine every row."""
import numpy as np
import pytest

import analogy_model as am
import util

pytestmark = pytest.mark.gpu

N, D, Q = 2080, 32, 70
CHAIN = {"prep", "sample", "threshold", "filter", "refine"}
KNN_KERNELS = {"exact_" + c for c in CHAIN}
JOIN_KERNELS = {"exact_join_" + c for c in CHAIN} | {"exact_join_gather"}
AN_KERNELS = {"analogy_" + c for c in CHAIN} | {"analogy_gather"}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def data(oracle):
    """The inputs and every expected list, computed once."""
    x = util.corpus(N, d=D).numpy().copy()
    ids = (np.arange(N) * 3 + 2).astype(np.int32)
    rng = np.random.default_rng(17)
    qs = rng.standard_normal((Q, D)).astype(np.float32)
    targets = ids[rng.choice(N, size=100, replace=False)]
    triples = ids[rng.integers(0, N, size=(40, 3))]
    knn32 = [oracle.exact_knn(x, ids, q, 32) for q in qs]
    join5 = [oracle.exact_knn(x, ids, q, 5, targets) for q in qs]
    x_t = np.ascontiguousarray(x.T)
    model = {m: am.model(x, ids, triples, 5, m, x_t=x_t) for m in ("3cosadd", "3cosmul")}
    return dict(x=x, ids=ids, qs=qs, targets=targets, triples=triples, knn32=knn32, join5=join5, model=model)


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    prof = {name: v[0] for name, v in idx.profile_read().items()}
    idx.profile_enable(False)
    return out, prof


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, np.nonzero((got[0] != exp[0]).any(1))[0][:8])
    assert np.array_equal(_bits(got[1]), _bits(exp[1])), (what, np.nonzero((_bits(got[1]) != _bits(exp[1])).any(1))[0][:8])


def _lists(exp, k):
    """The oracle's entries as (ids[Q][k], similarities[Q][k])."""
    return np.stack([e["id"][:k] for e in exp]).astype(np.int32), np.stack([e["dist"][:k] for e in exp]).astype(np.float32)


@pytest.mark.parametrize("check_brackets", [0, 4 | 8])
def test_knn_join_and_analogies_take_turns_on_one_handle(gpu, data, check_brackets):
    x, ids, qs, targets, triples = (data[n] for n in ("x", "ids", "qs", "targets", "triples"))

    def pin(join_tile=0):
        idx = gpu.VectorIndex(ids, x)
        idx.set_option("exact_filter", 1)
        idx.set_option("check_brackets", check_brackets)
        idx.set_option("exact_join_tile", join_tile)
        return idx

    def knn(k):
        return (lambda idx: idx.search(qs, k)), _lists(data["knn32"], k), KNN_KERNELS, {"exact_filter": 2, "exact_refine": 2}

    def join(tile):
        return (lambda idx: idx.join(qs, 5, targets)), _lists(data["join5"], 5), JOIN_KERNELS, {"exact_join_filter": 1, "exact_join_refine": 1}, tile

    def analogy(method):
        return (lambda idx: idx.analogy(triples, k=5, method=method)), data["model"][method], AN_KERNELS, {"analogy_filter": 2, "analogy_refine": 2}

    shared = pin()
    for step, (call, exp, kernels, launches, *tile) in enumerate([knn(5), join(0), analogy("3cosadd"), knn(32), analogy("3cosmul"), join(64)]):
        tile = tile[0] if tile else 0
        shared.set_option("exact_join_tile", tile)
        got, prof = _profiled(shared, lambda: call(shared))
        assert set(prof) == kernels, (step, sorted(prof))                # the filter's kernels and no all-exact scan
        assert all(prof[name] == n for name, n in launches.items()), (step, prof)
        own = pin(tile)
        alone = call(own)
        own.close()
        _same(got, alone, (step, "against a handle of its own"))
        _same(got, exp, (step, "against the oracle"))
    assert shared.last_join_stats()["redone_queries"] == 0 and shared.bound_violations() == 0
    shared.close()
