"""-m gpu: randomised soak of the re-ranking entry points with a FIXED seed budget (the long version is tools/soak_rerank.py): an
IVFIndex or a PQIndex and the VectorIndex of most of the same rows (tests/soak_inputs.py: draw_rerank) -- search_pv with k * pvf
on either side of every threshold of pv.h, the approximate analogies with n_cand from 4 to 4096, PQIndex.assign and
PQIndex.search_pv over a subset, with ids that have no vector row, a triple that is not searched and one whose sum is zero.
Lists and similarity bits equal pv_model / approx_analogy_model / assign_model; last_pv_stats and last_approx_analogy_stats equal
the counts the models give.  tests/test_soak_inputs_cpu.py proves which regimes the seed list reaches."""
import pytest

import assign_model
import pv_model as pm
import soak_inputs as si

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _pv_same(idx, got, pv, k, what):
    pm.same(got[0], got[1], pv["exp"], k, what)
    assert idx.last_pv_stats() == {"candidates": int(pv["candidates"].sum()), "scored": int(pv["scored"].sum())}, what


def run(gpu, d):
    what = d["label"]
    vec = gpu.VectorIndex(*d["vec_pin"])
    qs, t = d["qs"], d["triples"]
    if d["kind"] == "ivf":
        idx = gpu.IVFIndex(*d["pin"])
        calls = (("search_pv", lambda: _pv_same(idx, idx.search_pv(vec, qs, d["k"], d["pvf"], d["W"]), d["pv"], d["k"], what + " @ search_pv")),
                 ("analogy", lambda: idx.analogy(vec, t, d["ka"], d["n_cand"], d["W"])))
    else:
        idx = gpu.PQIndex(*d["pin"])
        calls = (("search_pv", lambda: _pv_same(idx, idx.search_pv(vec, qs, d["k"], d["pvf"], sentinel=100.0), d["pv"], d["k"], what + " @ search_pv")),
                 ("analogy", lambda: idx.analogy(vec, t, d["ka"], d["n_cand"])),
                 ("assign", lambda: idx.assign(qs, d["assign_targets"], sentinel=d["assign_sentinel"])),
                 ("search_pv subset", lambda: _pv_same(idx, idx.search_pv(vec, qs, d["k2"], d["pvf2"], sentinel=1000.0, subset_ids=d["subset"]),
                                                       d["pv2"], d["k2"], what + " @ search_pv subset")))
    for name, call in calls + calls[:2]:          # the first two once more: after the others have used the handle's buffers
        got = call()
        if name == "analogy":
            pm.same(got[0], got[1], d["analogy"]["exp"], d["ka"], what + " @ analogy")
            assert idx.last_approx_analogy_stats() == d["analogy"]["stats"], what + " @ analogy"
        elif name == "assign":
            assert assign_model.same(got, d["assign_exp"]), what + " @ assign"
    assert idx.bound_violations() == 0 and vec.bound_violations() == 0, what
    idx.close()
    vec.close()


@pytest.mark.parametrize("seed", si.SEEDS["rerank"])
def test_soak_rerank(gpu, oracle, seed):
    run(gpu, si.draw_rerank(seed, oracle))
