"""-m gpu: the HIP path through the C ABI against tests/golden/ref_*.npz -- stored tables and the lists the REFERENCE's own
set-returning functions returned over them (tests/golden/make_ref_golden.py).  Neither the oracle nor the reference build is
in the loop: ids and distance bits must equal the file's.  The handle's profile names the kernels that ran, so a fixture cannot
silently test a fallback:
    ref_d300_k256   K <= 256, one-byte codes: ivf_filter is fused8.h's whole-slab scan (option codes_u8 = 1, the default);
                    one query: ivf_one_kernel / pq_one_kernel (64 blocks of rows)
    ref_d300_k300   K > 256: ivf_filter can only be fused5.h's two-byte instantiation, with refine.h's merge_refine
    ref_d25_k256    m = 5: multi.h's ivf_multi_kernel
Batches here have 20 queries, below the 256 (query, cell) items from which the cell-grouped scans run by themselves, so the
batch calls set option fused = 1; single queries run with the defaults."""
import os

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_LIST = 5


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


def _load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    t = {k: z[k] for k in z.files}
    C = t["coarse"].shape[0]
    order = np.lexsort((t["ids"], t["cell"]))
    t["list_off"] = np.zeros(C + 1, np.int32)
    t["list_off"][1:] = np.cumsum(np.bincount(t["cell"], minlength=C))
    t["ivf_ids"], t["ivf_codes"], t["C"] = t["ids"][order], t["codes"][order], C
    return t


# name -> (kernels of a batched ivfadc search, of one ivfadc query, of a batched pq search, of one pq query)
FAMILY = {"ref_d300_k256": ({"ivf_filter", "merge_refine"}, {"ivf_one"}, {"pq_front", "ivf_filter"}, {"pq_one"}),
          "ref_d300_k300": ({"ivf_filter", "merge_refine"}, {"ivf_one"}, {"pq_front", "ivf_filter"}, {"lut_build", "adc_scan"}),
          "ref_d25_k256": ({"ivf_multi_scan", "merge_surv"}, {"lut_build", "adc_scan"}, {"lut_build", "adc_scan"}, {"lut_build", "adc_scan"})}
NEVER = {"ref_d300_k256": {"ivf_multi_scan"}, "ref_d300_k300": {"ivf_multi_scan"}, "ref_d25_k256": {"ivf_filter", "ivf_one", "pq_one", "pq_front"}}


@pytest.mark.parametrize("name", sorted(FAMILY))
def test_ivfadc_search_equals_the_reference(gpu, name):
    t = _load(name)
    batch_k, one_k, _, _ = FAMILY[name]
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ivf_ids"], t["ivf_codes"])
    qs = t["queries"]
    for W in (1, 3, t["C"]):
        exp = t[f"ivfadc_search_w{W}"]
        idx.set_option("fused", 1)
        (gi, gd), names = _profiled(idx, lambda: idx.search(qs, K_LIST, W, sentinel=1000.0, found_rule=gpu.FOUND_ROWS))
        print(name, "ivfadc batch W", W, sorted(names))
        util.assert_same_lists(gi, gd, exp, f"{name} ivfadc_search batch W={W}")
        assert batch_k <= names and not names & NEVER[name], (name, W, sorted(names))
        idx.set_option("fused", -1)
        for qi in (0, 4, 17):                                        # a row, its exact duplicate, a vector that is no row
            (gi, gd), names = _profiled(idx, lambda: idx.search(qs[qi:qi + 1], K_LIST, W, sentinel=1000.0, found_rule=gpu.FOUND_ROWS))
            print(name, "ivfadc one W", W, sorted(names))
            util.assert_same_lists(gi, gd, exp[qi:qi + 1], f"{name} ivfadc_search query {qi} W={W}")
            assert one_k <= names and not names & NEVER[name], (name, W, qi, sorted(names))
    # ivfadc_batch_search itself: W = 1, the accepted-rows rule, sentinel 100, the queries in fetch order
    fetched = t["vecs"][np.searchsorted(t["vec_ids"], t["batch_query_ids"])]
    idx.set_option("fused", 1)
    (gi, gd), names = _profiled(idx, lambda: idx.search(fetched, K_LIST, 1, sentinel=100.0, found_rule=gpu.FOUND_BATCH_UDF))
    print(name, "batch udf", sorted(names))
    util.assert_same_lists(gi, gd, t["ivfadc_batch_search"], f"{name} ivfadc_batch_search")
    assert batch_k <= names and not names & NEVER[name], (name, sorted(names))
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("name", sorted(FAMILY))
def test_pq_search_subset_and_grouping_equal_the_reference(gpu, name):
    t = _load(name)
    _, _, batch_k, one_k = FAMILY[name]
    idx = gpu.PQIndex(t["codebook"], t["ids"], t["pq_codes"])
    qs = t["queries"]
    (gi, gd), names = _profiled(idx, lambda: idx.search(qs, K_LIST, sentinel=100.0))
    print(name, "pq batch", sorted(names))
    util.assert_same_lists(gi, gd, t["pq_search"], f"{name} pq_search batch")
    assert batch_k <= names and not names & NEVER[name], (name, sorted(names))
    for qi in (0, 4, 17):
        (gi, gd), names = _profiled(idx, lambda: idx.search(qs[qi:qi + 1], K_LIST, sentinel=100.0))
        print(name, "pq one", sorted(names))
        util.assert_same_lists(gi, gd, t["pq_search"][qi:qi + 1], f"{name} pq_search query {qi}")
        assert one_k <= names and not names & NEVER[name], (name, qi, sorted(names))
    # pq_search_in: the subset (duplicates and unknown ids in it), sentinel 1000
    for lo, hi in ((0, 20), (4, 5)):
        (gi, gd), names = _profiled(idx, lambda: idx.search(qs[lo:hi], K_LIST, sentinel=1000.0, subset_ids=t["subset"]))
        print(name, "pq subset", sorted(names))
        util.assert_same_lists(gi, gd, t["pq_search_in"][lo:hi], f"{name} pq_search_in {lo}:{hi}")
        assert "gather_rows" in names, sorted(names)
    # grouping_pq: the subset and the whole table; two of the groups are the same vector
    for sub, key in ((t["subset"], "grouping"), (None, "grouping_all")):
        (gi, gg), names = _profiled(idx, lambda: idx.grouping(t["group_vecs"], sub))
        assert "grouping" in names, sorted(names)
        assert np.array_equal(gi, t[key + "_ids"]) and np.array_equal(gg, t[key + "_group"]), (name, key)
    idx.close()
