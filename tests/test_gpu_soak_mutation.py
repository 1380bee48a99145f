"""-m gpu: randomised soak of the four ways a pinned handle changes, with a FIXED seed budget (the long version is
tools/soak_mutation.py): per handle kind and seed one walk of ten steps (tests/soak_inputs.py: draw_mutation) -- append_rows,
remove_rows, update_rows and update_codebook in a drawn order with sizes from {1, 63, 64, 65, 300}, ids of pinned, earlier removed
and never known rows, and one call that must be refused.  After every step freddy_gpu_index_bytes equals a fresh pin's (a vector handle's lies in the window its buffer policy gives) and the
kind's search equals the oracle on the model's tables; at three drawn steps and the last, the full per-kind check of
tests/test_gpu_mutation.py runs and every answer equals a fresh pin's bit for bit.  The refused step raises FreddyGpuError where
the model raises Refused, and leaves nbytes, N and the answers as they were.  The vector walk runs with exact_filter = 1.
tests/test_soak_inputs_cpu.py proves which regimes the seed list reaches."""
import numpy as np
import pytest

import soak_inputs as si
import test_gpu_mutation as tm
import test_gpu_removal as tr
import test_gpu_update as tu
import update_model as um
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


PQ_ONE_BLOCKS = 64      # pq.hip, pq_one_shape: "n_blocks >= 64" (a literal there) -- the walks start on either side of it


def _cls(gpu, kind):
    return {"pq": gpu.PQIndex, "ivf": gpu.IVFIndex, "ivpq": gpu.IVPQIndex, "vec": gpu.VectorIndex}[kind]


def _search(kind, idx, qs, targets):
    """the walk's search -> (ids, floats[, iterations])"""
    if kind == "pq":
        return idx.search(qs, 7, sentinel=100.0)
    if kind == "ivf":
        return idx.search(qs, 5, 3)
    if kind == "ivpq":
        k, alpha, pvf, method = si.IVPQ_JOIN
        return idx.knn_join(qs, k, targets, alpha, pvf, method)
    return idx.search(qs, 5)


def _same_as_oracle(kind, got, exp, what):
    if kind == "ivpq":
        assert got[2] == exp[1], (what, "iterations", got[2], exp[1])
        util.assert_same_lists(got[0], got[1], exp[0], what)
    elif kind == "vec":
        tm._exact_same(got[0], got[1], exp, 5, what)
    else:
        util.assert_same_lists(got[0], got[1], exp, what)


def _apply(kind, idx, step):
    """one step on the handle -> what the call returns"""
    if step["call"] == "codebook":
        return idx.update_codebook(step["codebook"])
    if step["call"] == "remove":
        return idx.remove_rows(step["ids"])
    p = step["payload"]
    if step["call"] == "append":
        return idx.append_rows(step["ids"], coarse_id=p["coarse_id"], codes=p["codes"], vectors=p["vectors"])
    return idx.update_rows(step["ids"], coarse_id=p["coarse_id"], codes=p["codes"], vectors=p["vectors"])


def _full(gpu, oracle, kind, idx, model, d, step, what):
    """the per-kind check of tests/test_gpu_mutation.py, and bit equality with a fresh pin"""
    qs = d["qs"]
    rng = np.random.default_rng(len(what))
    ids = si.model_ids(kind, model)
    sub = np.concatenate([rng.choice(ids, size=min(ids.size, 300), replace=False), ids[:25], [1, -5, 10 ** 8 + 1]]).astype(np.int32)
    if kind == "pq":
        gv = qs[:5].copy()
        gv[3] = gv[0]
        if (model.N + 63) // 64 >= PQ_ONE_BLOCKS:
            tm._pq_check(gpu, oracle, idx, model, qs, sub, gv, True, what)
        else:                                   # fewer blocks than pq_one_kernel takes: the kernels a fresh pin is served by
            tu._pq_check_like_fresh(gpu, oracle, idx, model, qs, sub, gv, what)
    elif kind == "ivf":
        tm._ivf_check(gpu, oracle, idx, model, qs, True, True, what)
    elif kind == "vec":
        triples = ids[rng.integers(0, ids.size, size=(6, 3))].copy()
        triples[2, 0] = 10 ** 8 + 1
        tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, what, modes=(1,))
    fresh = _cls(gpu, kind)(*model.pin_args())
    if kind == "vec":
        fresh.set_option("exact_filter", 1)
    a, b = _search(kind, idx, qs, step["targets"]), _search(kind, fresh, qs, step["targets"])
    tm._bits_equal(a, b, what)
    if kind == "ivpq":
        assert a[2] == b[2], what
        for method, tl in ((0, True), (2, False)):
            a = idx.knn_join(qs, 10, step["targets"], 1, 3, method, use_target_lists=tl, confidence=0.3)
            b = fresh.knn_join(qs, 10, step["targets"], 1, 3, method, use_target_lists=tl, confidence=0.3)
            exp, it = oracle.ivpq_search_in(model.oracle_table(oracle), qs, 10, step["targets"], 1, 3, method, use_target_lists=tl, confidence=0.3)
            util.assert_same_lists(a[0], a[1], exp, what)
            tm._bits_equal(a, b, what)
            assert a[2] == b[2] == it, what
    if kind != "ivpq":
        assert idx.bound_violations() == 0 and fresh.bound_violations() == 0, what
    fresh.close()


def _fragment_bytes(model):
    """bytes of the exact filter's fragment-order copy of the model's rows (tests/test_gpu_mutation.py,
    test_index_bytes_of_an_ivpq_and_a_vec_handle_follow_the_tables)"""
    d = model.vectors.shape[1]
    return ((model.N + 31) // 32) * ((d + 15) // 16) * 2 * 64 * 16


def _vec_bytes(gpu, idx, model, need_max, what):
    """freddy_gpu_index_bytes of a vector handle against a fresh pin's.  xb, the row-major copy and the ids are held at their exact
    size; the fragment-order copy is a DevBuf (internal.h, DevBuf::ensure), which allocates f(need) = need + need / 8 + 256 bytes
    when it has to grow and keeps a buffer that is large enough.  A fresh pin holds f(need) for the rows there are now; the walked
    handle holds at least need and at most f of the largest need the walk has seen:
        fresh - (need / 8 + 256)  <=  walked  <=  fresh + f(need_max) - f(need)"""
    f = lambda n: n + n // 8 + 256
    need = _fragment_bytes(model)
    fresh = gpu.VectorIndex(*model.pin_args())
    lo, hi = fresh.nbytes - (need // 8 + 256), fresh.nbytes + f(need_max) - f(need)
    assert lo <= idx.nbytes <= hi, (what, "freddy_gpu_index_bytes", lo, idx.nbytes, hi)
    fresh.close()


def run(gpu, oracle, d):
    kind = d["kind"]
    model = si.mutation_model(kind, d["start"])
    idx = _cls(gpu, kind)(*model.pin_args())
    if kind == "vec":
        idx.set_option("exact_filter", 1)
    need_max = _fragment_bytes(model) if kind == "vec" else 0
    for si_, step in enumerate(d["steps"]):
        what = f"{d['label']} @ step {si_}"
        if step["op"] == "refused":
            was, nbytes, n = _search(kind, idx, d["qs"], step["targets"]), idx.nbytes, idx.N
            with pytest.raises(gpu.FreddyGpuError, match=tm.E_ARG):
                _apply(kind, idx, step)
            with pytest.raises(um.Refused):
                si.apply_to_model(kind, model, step)
            assert idx.nbytes == nbytes and idx.N == n == model.N, what
            now = _search(kind, idx, d["qs"], step["targets"])
            tm._bits_equal(was, now, what + " (after the refused call)")
        else:
            got, exp = _apply(kind, idx, step), si.apply_to_model(kind, model, step)
            assert got == exp == step["returns"], (what, got, exp, step["returns"])
        assert idx.N == model.N == step["N"], what
        if kind == "vec":
            need_max = max(need_max, _fragment_bytes(model))
            _vec_bytes(gpu, idx, model, need_max, what)
        else:
            tr._same_bytes(idx, _cls(gpu, kind), model, what)
        _same_as_oracle(kind, _search(kind, idx, d["qs"], step["targets"]), step["exp"], what)
        if step["full"]:
            _full(gpu, oracle, kind, idx, model, d, step, what)
    assert si.model_bytes(kind, model) == d["final_bytes"], d["label"]
    idx.close()


@pytest.mark.parametrize("seed", si.SEEDS["mutation"])
@pytest.mark.parametrize("kind", si.MUTATION_KINDS)
def test_soak_mutation(gpu, oracle, kind, seed):
    run(gpu, oracle, si.draw_mutation(kind, seed, oracle))
