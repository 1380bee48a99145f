"""-m gpu: randomised soak of the exact entry points with a FIXED seed budget (the long version is tools/soak_exact.py): one
VectorIndex per seed (tests/soak_inputs.py: draw_exact), 6 - 8 calls in a random order on the same handle -- search, search over a
subset, the exact join, exact_assign and the three analogy methods share verdict words, counters and candidate buffers.  After
every call the ids and the similarity bits equal the oracle's / the numpy models', bound_violations() == 0, and where every row
is refined (option check_brackets bits 2 and 3) and the filter serves the call, bound_checked() grew.
tests/test_soak_inputs_cpu.py proves which regimes the seed list reaches."""
import numpy as np
import pytest

import assign_model
import soak_inputs as si
import test_gpu_exact_join as tj

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def filter_serves(d, call):
    """Whether filter + refine answers the call (exf_wanted, exact_host.h, and want_filter of the three entry points in exact.hip / analogy.hip; analogy.h: an_filter_lds): the
    condition under which a refine-all run must have compared rows with their brackets."""
    if not si.filter_eligible(d["d"]):
        return False
    forced = d["exact_filter"] == 1
    kind = call["kind"]
    if kind == "search":
        return d["k"] <= 32 and (forced or d["N"] >= si.EXF_AUTO_ROWS)
    if kind == "join":
        n = np.intersect1d(call["ids"], d["ids"]).size
        return d["k"] <= 32 and n >= 1 and (forced or n >= si.exj_min_targets())
    if kind in ("3cosadd", "3cosmul"):
        tiles = 3 if kind == "3cosmul" else 1
        fits = tiles * ((d["d"] + 15) // 16) * 2 * 64 * 16 <= 160 * 1024
        live = np.isin(call["triples"], d["ids"]).all(1).any()
        return call["ids"] is None and fits and live and (forced or d["N"] >= si.EXF_AUTO_ROWS)
    return False


def run(gpu, d):
    """every call of the draw on one handle"""
    idx = gpu.VectorIndex(d["ids"], d["x"])
    idx.set_option("exact_filter", d["exact_filter"])
    if d["refine_all"]:
        idx.set_option("check_brackets", 4 | 8)
    k, qs = d["k"], d["qs"]
    for ci, c in enumerate(d["calls"]):
        what = f"{d['label']} @ call {ci}: {c['kind']}"
        checked = idx.bound_checked()
        kind = c["kind"]
        if kind == "search":
            gi, gs = idx.search(qs, k)
            tj._same(gi, gs, c["exp"], k, what)
        elif kind == "search_subset":
            gi, gs = idx.search(qs, k, subset_ids=c["ids"])
            tj._same(gi, gs, c["exp"], k, what)
        elif kind == "join":
            gi, gs = idx.join(qs, k, c["ids"])
            tj._same(gi, gs, c["exp"], k, what)
        elif kind == "assign":
            assert assign_model.same(idx.assign(qs, c["ids"]), c["exp"]), what
        else:
            gi, gs = idx.analogy(c["triples"], k=c["k"], method=kind, subset_ids=c["ids"])
            ei, es = c["exp"]
            assert np.array_equal(gi, ei), (what, np.nonzero((gi != ei).any(1))[0][:5])
            assert np.array_equal(gs.view(np.uint64), es.view(np.uint64)), (what, np.nonzero((gs.view(np.uint64) != es.view(np.uint64)).any(1))[0][:5])
        assert idx.bound_violations() == 0, what
        if d["refine_all"] and filter_serves(d, c):
            assert idx.bound_checked() > checked, (what, "every row is to be refined, and none was checked")
    idx.close()


@pytest.mark.parametrize("seed", si.SEEDS["exact"])
def test_soak_exact(gpu, oracle, seed):
    run(gpu, si.draw_exact(seed, oracle))
