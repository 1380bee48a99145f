"""-m gpu: every path of the IVFADC units (ivfadc.hip and the units it calls) and pq.hip taking turns on handles that are pinned ONCE.  The paths size and overwrite the same
workspace of their handle (items, counters, survivor regions, the query table and its compact copy, the partial lists, the
one-launch buffer), and a flat-PQ batch runs the IVFADC filter + refine chain on a run state of its own making; a fixed sequence
of calls is run forward and then backward, so every path follows every kind of neighbour.  Every call's lists must be bit for bit
the CPU oracle's, and the labels in its profile must be exactly the launches its path is documented to make:
a call that quietly took another path, or an extra probing round, shows.

The smallest shapes that reach each path (thresholds: ivfadc_begin, pq_use_fused, pq_fused_chunk, bigk.h):
    main     d = 300, m = 12, K = 256, 6 000 rows (94 row blocks: one full pseudo-list of 4096 rows and a short one), 16 cells;
             Q = 32 (the tiled coarse kernels: one coarse + table launch) and Q = 3 (table and coarse kernels apart), k = 5, W = 3
    k = 513  the generic scan's selection passes (2k > 1024); W = 8: every query's eight nearest cells hold >= 1026 rows
    K = 1024 the FULLK instantiations (20 000 rows, 32 cells: the table the parity tests build)
    d = 25   m = 5: multi.h (tests/golden/ref_d25_k256.npz)
    sliced   33 pseudo-lists = 131 073 rows (pq_fused_chunk: >= 32 lists and more than 256 survivor regions per query): the main
             table's code rows repeated under new ids, so most distances are shared by 21 rows
"""
import os

import numpy as np
import pytest

import util
from freddy_amd import index_build as ib

pytestmark = pytest.mark.gpu

N, C, K_LIST, W = 6000, 16, 5, 3
N_BIG = 32 * 4096 + 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_d25_k256.npz")

# the launches of a call, by path
FRONT_TILED = {"coarse_table"}                       # Q >= 32 with the filter scan: MFMA cell selection + query table, one launch
FRONT_SMALL = {"query_codebook", "coarse_dist"}      # fewer queries: the table kernel, then the coarse kernel
FILTER = {"probe_plan", "work_table", "entry_records", "ivf_filter", "merge_refine"}
EXACT = {"coarse_dist", "probe_plan", "work_table", "ivf_exact_scan", "merge_surv"}
MULTI = {"coarse_dist", "probe_plan", "work_table", "lut_build", "ivf_multi_scan", "merge_surv"}
GENERIC = {"coarse_dist", "probe_plan", "lut_build", "adc_scan", "merge_replay"}
BIGK = {"coarse_dist", "probe_plan", "lut_build", "adc_scan", "merge_select", "bigk_replay"}
PQ_FUSED = {"pq_front", "ivf_filter", "merge_refine"}
PQ_GENERIC = {"lut_build", "adc_scan", "merge_replay"}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _ivf_expect(oracle, t, qs, k, w, rule):
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    return oracle.ivfadc_search_many(ot, qs, k, w, sentinel=1000.0, found_rule=rule)


@pytest.fixture(scope="module")
def data(oracle):
    """The tables, the queries and every expected list, computed once."""
    d = {}
    x = util.corpus(N)   # (a short training: the codebooks' quality is not what these calls test)
    ivf = ib.build_ivf_index(x, C=C, m=12, K=256, train_size=2000, iters=2, seed=5)
    pq = ib.build_pq_index(x, m=12, K=256, train_size=2000, iters=2, seed=6)
    _, qs = util.queries_from_corpus(N, 32, seed=41)
    d.update(ivf=ivf, pq=pq, qs=qs)
    for nq in (32, 3, 1):
        for rule in (0, 1):
            d["ivf", nq, rule] = _ivf_expect(oracle, ivf, qs[:nq], K_LIST, W, rule)
    lo = np.asarray(ivf["list_off"], np.int64)
    cells = np.argsort(((qs[:, None, :] - ivf["coarse"][None]) ** 2).sum(-1), axis=1)[:, :8]
    assert (lo[cells + 1] - lo[cells]).sum(1).min() >= 2 * 513, "k = 513 needs 2k rows in every query's probe set"
    d["ivf_bigk"] = _ivf_expect(oracle, ivf, qs, 513, 8, 0)
    ivf1024 = util.ivf_tables(N=20000, C=32, K=1024)
    _, qs1024 = util.queries_from_corpus(20000, 32, seed=43)
    d.update(ivf1024=ivf1024, qs1024=qs1024)
    for rule in (0, 1):
        d["ivf1024", rule] = _ivf_expect(oracle, ivf1024, qs1024, K_LIST, W, rule)
    z = np.load(GOLDEN)
    order = np.lexsort((z["ids"], z["cell"]))
    off = np.zeros(z["coarse"].shape[0] + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(z["cell"], minlength=z["coarse"].shape[0]))
    d25 = dict(coarse=z["coarse"], codebook=z["codebook"], list_off=off, ids=z["ids"][order], codes=z["codes"][order])
    d.update(d25=d25, qs25=z["queries"])
    d["ivf25"] = _ivf_expect(oracle, d25, z["queries"], K_LIST, W, 0)
    # the flat table
    pt = oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"])
    d["pq", 16] = np.stack([oracle.pq_search(pt, q, K_LIST) for q in qs[:16]])
    rng = np.random.default_rng(7)
    for n_sub in (4500, 1500):   # 71 row blocks: a pseudo-list and a short one; 24 blocks: the generic scan
        ids = rng.choice(pq["ids"], size=n_sub, replace=False).astype(np.int32)
        d["subset", n_sub] = ids
        d["pq_in", n_sub] = oracle.pq_search_in_batch(pt, qs[:16], K_LIST, ids, use_target_lists=True)
    reps = -(-N_BIG // N)
    big_codes = np.ascontiguousarray(np.tile(pq["codes"], (reps, 1))[:N_BIG])
    big_ids = np.arange(1, N_BIG + 1, dtype=np.int32)
    d.update(big_codes=big_codes, big_ids=big_ids)
    bt = oracle.pq_table(pq["codebook"], big_ids, big_codes)
    d["pq_big"] = np.stack([oracle.pq_search(bt, q, K_LIST) for q in qs[:16]])
    return d


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    launches = {name: v[0] for name, v in idx.profile_read().items()}
    idx.profile_enable(False)
    return out, launches


def _options(idx, **opts):
    for name, value in opts.items():
        idx.set_option(name, value)


def test_every_path_takes_turns_on_handles_pinned_once(gpu, data):
    qs, qs1024, qs25 = data["qs"], data["qs1024"], data["qs25"]
    pin_ivf = lambda t: gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    h = dict(ivf=pin_ivf(data["ivf"]), ivf1024=pin_ivf(data["ivf1024"]), ivf25=pin_ivf(data["d25"]),
             pq=gpu.PQIndex(data["pq"]["codebook"], data["pq"]["ids"], data["pq"]["codes"]),
             pq_big=gpu.PQIndex(data["pq"]["codebook"], data["big_ids"], data["big_codes"]))
    for name in ("ivf", "ivf1024", "ivf25"):
        _options(h[name], coarse_approx=1, running_bound=1)
    RULE = {0: gpu.FOUND_ROWS, 1: gpu.FOUND_ACCEPTED}

    def ivf(handle, queries, exp, labels, k=K_LIST, w=W, rule=0, **opts):
        opts = dict(dict(fused=1, fused_kernel=5, codes_u8=1, sparse_items=0), **opts)
        def call():
            _options(h[handle], **opts)
            return h[handle].search(queries, k, w, sentinel=1000.0, found_rule=RULE[rule])
        return (handle, sorted(opts.items()), len(queries), k, w, rule), handle, call, exp, labels

    def pq(handle, queries, exp, labels, subset=None, sentinel=100.0, **opts):
        opts = dict(dict(pq_fused=-1), **opts)
        def call():
            _options(h[handle], **opts)
            return h[handle].search(queries, K_LIST, sentinel=sentinel, subset_ids=subset)
        return (handle, sorted(opts.items()), len(queries), None if subset is None else len(subset)), handle, call, exp, labels

    # the filter + refine scan: ivf_filter8 / the one-byte ivf_filter5 / the int16 ivf_filter5, both found rules, the item and pair kernels
    scans = []
    for i, (u8, rule, sparse) in enumerate((u8, rule, sparse) for u8 in (1, 2, 0) for rule in (0, 1) for sparse in (0, -1, -2)):
        nq = (32, 3)[i % 2]
        labels = (FRONT_TILED if nq == 32 else FRONT_SMALL) | FILTER | ({"sparse_items"} if sparse else set())
        scans.append(ivf("ivf", qs[:nq], data["ivf", nq, rule], labels, rule=rule, codes_u8=u8, sparse_items=sparse))
    others = [
        pq("pq", qs[:16], data["pq", 16], PQ_FUSED, pq_fused=1),
        # one query, the defaults (fused = -1: by the batch's size): the one-launch kernel answers (verdict 2), or asks for the
        # multi-round path (3), or -- after a grid that once did not become co-resident -- is not tried: the list is the oracle's
        ivf("ivf", qs[:1], data["ivf", 1, 0], None, fused=-1),
        ivf("ivf", qs, data["ivf", 32, 0], EXACT, fused_kernel=3),
        pq("pq", qs[:16], data["pq", 16], PQ_GENERIC, pq_fused=0),
        ivf("ivf", qs, data["ivf", 32, 1], GENERIC, rule=1, fused=0),
        pq("pq_big", qs[:16], data["pq_big"], PQ_FUSED | {"merge_replay"}),                        # the sliced merge
        ivf("ivf", qs, data["ivf_bigk"], BIGK, k=513, w=8, fused=0),
        pq("pq", qs[:16], data["pq_in", 4500], PQ_FUSED | {"gather_rows"}, subset=data["subset", 4500], sentinel=1000.0),
        ivf("ivf", qs[:1], data["ivf", 1, 1], None, rule=1, fused=-1),
        ivf("ivf25", qs25, data["ivf25"], MULTI),
        pq("pq", qs[:16], data["pq_in", 1500], PQ_GENERIC | {"gather_rows"}, subset=data["subset", 1500], sentinel=1000.0),
        ivf("ivf", qs[:3], data["ivf", 3, 0], EXACT, fused_kernel=3),
        # K = 1024: the FULLK instantiations of the int16 scan (both found rules), the exact scan and the generic scan
        ivf("ivf1024", qs1024, data["ivf1024", 0], FRONT_TILED | FILTER),
        ivf("ivf1024", qs1024, data["ivf1024", 1], FRONT_TILED | FILTER, rule=1),
        ivf("ivf1024", qs1024, data["ivf1024", 0], EXACT, fused_kernel=3),
        ivf("ivf1024", qs1024, data["ivf1024", 0], GENERIC, fused=0),
    ]
    calls = [c for pair in zip(scans, others + [None] * (len(scans) - len(others))) for c in pair if c is not None]
    assert len(calls) == len(scans) + len(others)

    for direction, sequence in (("forward", calls), ("backward", calls[::-1])):
        for step, (what, handle, call, exp, labels) in enumerate(sequence):
            (gi, gd), launches = _profiled(h[handle], call)
            print(direction, step, what, sorted(launches.items()))
            names = set(launches)
            util.assert_same_lists(gi, gd, exp, f"{direction} step {step}: {what}")
            if labels is None:
                assert names in ({"ivf_one"}, {"ivf_one"} | GENERIC, GENERIC), (direction, step, what, sorted(names))
            else:
                assert names == labels, (direction, step, what, sorted(names), sorted(labels))
    for name, idx in h.items():
        assert idx.bound_violations() == 0, name
        idx.close()
