"""tests/golden/ref_*.npz hold stored tables and what the REFERENCE's set-returning functions returned over them
(tests/golden/make_ref_golden.py).  Here the fresh oracle, and the fresh reference build where it exists, reproduce the files
bit for bit; tests/test_gpu_ref_golden.py holds the HIP path to the same files."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ref_golden as mk  # noqa: E402
import ref_fixture as rf  # noqa: E402
from oracle import ref as R  # noqa: E402

FILES = sorted(glob.glob(os.path.join(HERE, "golden", "ref_*.npz")))
K_LIST = mk.K_LIST


def same(a, b, what):
    assert np.array_equal(a["id"], b["id"]), what
    assert np.array_equal(a["dist"].view(np.uint32), b["dist"].view(np.uint32)), what


def test_the_three_fixtures_exist_and_are_small():
    assert [os.path.basename(f)[:-4] for f in FILES] == sorted(mk.SHAPES)
    for f in FILES:
        assert os.path.getsize(f) <= 500 * 1000, f
        z = np.load(f)
        m, K, s = z["codebook"].shape
        shape = mk.SHAPES[os.path.basename(f)[:-4]]
        assert (m * s, m, K, z["coarse"].shape[0], z["ids"].size) == tuple(shape[k] for k in ("d", "m", "K", "C", "N"))
        assert z["queries"].shape[0] == 20 and z["query_ids"].size == 16
        # exact duplicate rows: equal codes in both indexes for at least 1 % of the rows
        both = np.concatenate([z["pq_codes"], z["codes"], z["cell"][:, None].astype(np.int16)], axis=1)
        assert z["ids"].size - np.unique(both, axis=0).shape[0] >= z["ids"].size // 100


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_oracle_reproduces_the_reference_fixture(oracle, path):
    z = np.load(path)
    t = mk.tables_from_file(z)
    pq_t, ivf_t = rf.oracle_tables(oracle, t)
    qs = t["queries"]
    same(np.stack([oracle.pq_search(pq_t, q, K_LIST) for q in qs]), z["pq_search"], "pq_search")
    same(np.stack([oracle.pq_search_in(pq_t, q, K_LIST, t["subset"]) for q in qs]), z["pq_search_in"], "pq_search_in")
    for W in (1, 3, t["C"]):
        same(oracle.ivfadc_search_many(ivf_t, qs, K_LIST, W, sentinel=1000.0, found_rule=0), z[f"ivfadc_search_w{W}"], f"ivfadc_search W={W}")
    fetched = t["vecs"][np.searchsorted(t["vec_ids"], z["batch_query_ids"])]
    assert z["batch_query_ids"].tolist() == sorted(set(t["query_ids"].tolist()))
    same(oracle.ivfadc_batch_search(ivf_t, fetched, K_LIST), z["ivfadc_batch_search"], "ivfadc_batch_search")
    for ids, key in ((t["subset"], "grouping"), (t["ids"], "grouping_all")):
        gi, gg = oracle.grouping_pq(pq_t, t["group_vecs"], ids)
        assert np.array_equal(gi, z[key + "_ids"]) and np.array_equal(gg, z[key + "_group"]), key
    assert np.array_equal(t["group_vecs"], t["vecs"][np.searchsorted(t["vec_ids"], t["group_ids"])])
    assert np.array_equal(qs[:16], t["vecs"][np.searchsorted(t["vec_ids"], t["query_ids"])])


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_reference_build_reproduces_its_fixture(path):
    if R.status() == "absent":
        pytest.skip("neither the reference tree nor oracle/_ref exists")
    z = np.load(path)
    out = mk.reference_outputs(R.Ref(), mk.tables_from_file(z))
    for key, val in out.items():
        if val.dtype.names:
            same(val, z[key], key)
        else:
            assert np.array_equal(val, z[key]), key
