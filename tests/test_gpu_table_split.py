"""The query x codebook table on f16-split operands (csrc/fused5.h query_codebook5_body) at all three of its launch sites.

The table units form every dot product as three v_mfma_f32_16x16x32_f16 on operands scaled by a power of two per position
(codebook, pin time) and per (query, position).  What can go wrong there is the scaling (tiny and large codebooks, an all-zero
position, one codeword far above its neighbours, zero and one-hot sub-vectors) and the bracket E that has to cover the split's
error: with check_brackets = 3 the scan keeps and the merge refines EVERY probed row and cell and compares the exact distance
with its bracket, so a table word outside its proven error shows as a bound violation or as a list that differs from the CPU
oracle's.  Batches of 16, 17, 33 and 48 queries take coarse_table5_kernel (Q >= 32) and query_codebook5_kernel (fewer); a flat PQ
handle's 48 queries go through pq_front_kernel."""
import numpy as np
import pytest

import util
from freddy_amd import index_build as ib

pytestmark = pytest.mark.gpu

N, C, M, S, K_LIST, W, QMAX = 6000, 8, 12, 25, 5, 3, 48
ZERO_POS, SPIKE_POS, SPIKE_CODE = 3, 7, 5
# 2^-64, 2^-80, 2^-140: the small end of binary32.  The distances are quadratic: at 2^-64 they are around 2^-128, subnormal, from
# 2^-80 on most of them are 0 -- a list is decided by the scan order under massive ties, and the brackets have to hold all the same.
SCALES = {"2^-20": 2.0 ** -20, "1": 1.0, "2^12": 2.0 ** 12, "2^-64": 2.0 ** -64, "2^-80": 2.0 ** -80, "2^-140": 2.0 ** -140}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _doctor(codebook):
    """One position whose codewords are all zero, one with a single codeword 10^3 x its neighbours."""
    cb = np.array(codebook, np.float32).reshape(M, -1, S)
    cb[ZERO_POS] = 0.0
    cb[SPIKE_POS, SPIKE_CODE] *= 1e3
    return cb


@pytest.fixture(scope="module")
def base():
    """Per K: the IVF and the flat PQ tables over the same 6000 rows, and the queries -- indexed rows (the benchmark's kind), one
    with a zero sub-vector, one with a one-hot sub-vector."""
    x = util.corpus(N)
    _, qs = util.queries_from_corpus(N, QMAX, seed=77)
    qs = qs.copy()
    qs[1, 2 * S:3 * S] = 0.0
    qs[2, 4 * S:5 * S] = 0.0
    qs[2, 4 * S + 11] = 1.0
    qs[18, ZERO_POS * S:(ZERO_POS + 1) * S] = 0.0     # a zero sub-vector against the all-zero position
    qs[35, SPIKE_POS * S:(SPIKE_POS + 1) * S] = 0.0
    qs[35, SPIKE_POS * S] = -1.0                      # one-hot against the spike
    d = dict(qs=qs)
    for K in (1024, 256):
        ivf = ib.build_ivf_index(x, C=C, m=M, K=K, train_size=5000, iters=2, seed=5)
        pq = ib.build_pq_index(x, m=M, K=K, train_size=5000, iters=2, seed=6)
        d[K] = dict(ivf=dict(ivf, codebook=_doctor(ivf["codebook"]), plain=np.array(ivf["codebook"], np.float32)),
                    pq=dict(pq, codebook=_doctor(pq["codebook"])))
    return d


_EXPECTED = {}


def _variant(base, oracle, K, scale):
    """The tables and queries times `scale` (coarse centroids too: the same index in other units) and the oracle's lists, once."""
    key = (K, scale)
    if key not in _EXPECTED:
        s = np.float32(SCALES[scale])
        ivf, pq = base[K]["ivf"], base[K]["pq"]
        qs = base["qs"] * s
        sent = float(1000.0 * s * s)
        if 1000.0 * SCALES[scale] ** 2 < 2.0 ** -126:     # below binary32's normal range: the plain sentinel, or every list is fillers
            sent = 1000.0
        v = dict(qs=qs, sentinel=sent, coarse=ivf["coarse"] * s, codebook=ivf["codebook"] * s, plain=ivf["plain"] * s,
                 pq_codebook=pq["codebook"] * s)
        ot = oracle.ivf_table(v["coarse"], v["codebook"], ivf["list_off"], ivf["ids"], ivf["codes"])
        v["ivf"] = oracle.ivfadc_search_many(ot, qs, K_LIST, W, sentinel=sent, found_rule=0)
        pt = oracle.pq_table(v["pq_codebook"], pq["ids"], pq["codes"])
        v["pq"] = np.stack([oracle.pq_search(pt, q, K_LIST) for q in qs])
        _EXPECTED[key] = v
    return _EXPECTED[key]


def _head(exp, Q):
    return {"id": exp["id"].reshape(QMAX, K_LIST)[:Q], "dist": exp["dist"].reshape(QMAX, K_LIST)[:Q]}


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


def _ivf_options(idx):
    for name, value in dict(coarse_approx=1, running_bound=1, fused=1, fused_kernel=5, codes_u8=1, sparse_items=0).items():
        idx.set_option(name, value)


@pytest.mark.parametrize("scale", sorted(SCALES))
@pytest.mark.parametrize("K", [1024, 256])
def test_ivf_lists_and_brackets_at_both_launch_sites(gpu, oracle, base, K, scale):
    v = _variant(base, oracle, K, scale)
    t = base[K]["ivf"]
    idx = gpu.IVFIndex(v["coarse"], v["codebook"], t["list_off"], t["ids"], t["codes"])
    _ivf_options(idx)
    for Q in (16, 17, 33, 48):
        for brackets in (3, 0):
            idx.set_option("check_brackets", brackets)
            (gi, gd), names = _profiled(idx, lambda: idx.search(v["qs"][:Q], K_LIST, W, sentinel=v["sentinel"], found_rule=gpu.FOUND_ROWS))
            what = f"K {K} scale {scale} Q {Q} check_brackets {brackets}"
            assert ("coarse_table" in names) == (Q >= 32) and ("query_codebook" in names) == (Q < 32), (what, sorted(names))
            assert {"ivf_filter", "merge_refine"} <= names, (what, sorted(names))
            util.assert_same_lists(gi, gd, _head(v["ivf"], Q), what)
            assert idx.bound_violations() == 0, what
    # another codebook on the same handle: the fragment copy and its exponents are rebuilt -- the lists of a fresh pin
    idx.update_codebook(v["plain"])
    fresh = gpu.IVFIndex(v["coarse"], v["plain"], t["list_off"], t["ids"], t["codes"])
    _ivf_options(fresh)
    for Q in (17, 48):
        gi, gd = idx.search(v["qs"][:Q], K_LIST, W, sentinel=v["sentinel"], found_rule=gpu.FOUND_ROWS)
        fi, fd = fresh.search(v["qs"][:Q], K_LIST, W, sentinel=v["sentinel"], found_rule=gpu.FOUND_ROWS)
        assert np.array_equal(gi, fi) and np.array_equal(gd.view(np.uint32), fd.view(np.uint32)), f"K {K} scale {scale} Q {Q} after update_codebook"
    assert idx.bound_violations() == 0 and fresh.bound_violations() == 0
    idx.close()
    fresh.close()


@pytest.mark.parametrize("scale", sorted(SCALES))
@pytest.mark.parametrize("K", [1024, 256])
def test_flat_pq_batch_goes_through_pq_front(gpu, oracle, base, K, scale):
    v = _variant(base, oracle, K, scale)
    t = base[K]["pq"]
    idx = gpu.PQIndex(v["pq_codebook"], t["ids"], t["codes"])
    idx.set_option("pq_fused", 1)
    for brackets in (3, 0):
        idx.set_option("check_brackets", brackets)
        # (the oracle's pq_search has the reference's fixed sentinel, 100: at scale 2^12 every distance lies beyond it and the lists
        # are fillers on both sides -- the brackets of every row are checked all the same; the scaled sentinel is used below)
        (gi, gd), names = _profiled(idx, lambda: idx.search(v["qs"], K_LIST, sentinel=100.0))
        what = f"pq K {K} scale {scale} check_brackets {brackets}"
        assert {"pq_front", "ivf_filter", "merge_refine"} <= names, (what, sorted(names))
        util.assert_same_lists(gi, gd, v["pq"], what)
        assert idx.bound_violations() == 0, what
    plain = np.array(t["codebook"], np.float32) * np.float32(SCALES[scale])
    plain[ZERO_POS] = plain[ZERO_POS + 1]            # (no zero position any more: another exponent)
    idx.update_codebook(plain)
    fresh = gpu.PQIndex(plain, t["ids"], t["codes"])
    fresh.set_option("pq_fused", 1)
    gi, gd = idx.search(v["qs"], K_LIST, sentinel=v["sentinel"])
    fi, fd = fresh.search(v["qs"], K_LIST, sentinel=v["sentinel"])
    assert np.array_equal(gi, fi) and np.array_equal(gd.view(np.uint32), fd.view(np.uint32)), f"pq K {K} scale {scale} after update_codebook"
    assert idx.bound_violations() == 0 and fresh.bound_violations() == 0
    idx.close()
    fresh.close()
