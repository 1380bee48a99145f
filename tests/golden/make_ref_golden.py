"""Writes tests/golden/ref_*.npz: stored inputs and the REFERENCE's outputs.

Unlike freddy_small.npz (the oracle's own bits) the expected lists here were produced by the reference's C code: its
set-returning functions pq_search, pq_search_in, ivfadc_search, ivfadc_batch_search and grouping_pq, run to exhaustion over
the stored tables by oracle/_ref/libfreddy_ref.so (oracle/ref/).  Data only; each file stays under
500 KB (codebooks are rounded to multiples of 2^-12 so that they compress, and the flat PQ index shares the residual
codebook).  tests/test_ref_golden_cpu.py holds the fresh oracle and the fresh reference build to the files,
tests/test_gpu_ref_golden.py the HIP path, with neither in the loop.

    python tests/golden/make_ref_golden.py        # needs oracle/_ref (make -C oracle ref) and the oracle
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import ref_fixture as rf  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from oracle.ref import Ref  # noqa: E402

# name -> shape; the scan each one is for (tests/test_gpu_ref_golden.py asserts the kernels by name)
SHAPES = {"ref_d300_k256": dict(d=300, m=12, K=256, C=8, N=4200, seed=41),    # fused8.h, pq_one_kernel / ivf_one_kernel (64 blocks of rows)
          "ref_d300_k300": dict(d=300, m=12, K=300, C=8, N=2000, seed=42),    # two-byte codes: fused5.h + refine.h
          "ref_d25_k256": dict(d=25, m=5, K=256, C=32, N=2000, seed=43)}      # multi.h
K_LIST = 5


def build(o, d, m, K, C, N, seed):
    rng = np.random.default_rng(seed)
    t = rf.small_index(o, d, m, K, C, N, seed, dup=())
    x = t["x"]
    n_dup = N // 100                                                   # 1 % exact duplicates, re-encoded below
    src, dst = rng.choice(N // 2, n_dup, replace=False), N // 2 + rng.choice(N // 2, n_dup, replace=False)
    x[dst] = x[src]
    grid = np.float32(4096)
    t["codebook"] = (np.round(t["codebook"] * grid) / grid).astype(np.float32)
    t["pq_codebook"] = t["codebook"]
    t["pq_codes"] = o.encode_pq(t["pq_codebook"], x)
    t["cell"] = o.assign_coarse(t["coarse"], x).astype(np.int32)
    t["codes"] = o.encode_pq(t["codebook"], (x - t["coarse"][t["cell"]]).astype(np.float32))
    order = np.lexsort((t["ids"], t["cell"]))
    t["list_off"] = np.zeros(C + 1, np.int32)
    t["list_off"][1:] = np.cumsum(np.bincount(t["cell"], minlength=C))
    t["ivf_ids"], t["ivf_codes"] = t["ids"][order], t["codes"][order]
    inside = np.concatenate([src[:4], dst[:4], rng.choice(N, 8, replace=False)])       # rows with an exact duplicate among them
    outside = rng.standard_normal((4, d)).astype(np.float32)
    outside = (outside / np.linalg.norm(outside, axis=1, keepdims=True)).astype(np.float32)
    t["query_ids"] = t["ids"][inside]
    t["queries"] = np.concatenate([x[inside], outside])
    t["subset"] = np.concatenate([rng.choice(t["ids"], N // 3, replace=False), t["ids"][src[:6]], t["ids"][dst[:6]],
                                  np.array([7, 7, N + 3, -2])]).astype(np.int32)
    t["group_ids"] = np.array(sorted({int(t["ids"][src[0]]), int(t["ids"][dst[0]]), 5, N // 2, N - 1}), np.int32)   # two equal vectors
    t["group_vecs"] = x[t["group_ids"] - 1]
    t["vec_ids"] = np.union1d(t["query_ids"], t["group_ids"]).astype(np.int32)        # the rows of the vectors table that are fetched
    t["vecs"] = x[t["vec_ids"] - 1]
    t["x_rows"] = (t["vec_ids"], t["vecs"])
    return t


STORED = ("coarse", "codebook", "ids", "pq_codes", "cell", "codes", "queries", "query_ids", "subset", "group_ids", "group_vecs", "vec_ids", "vecs")


def reference_outputs(r, t):
    """What the reference's SRFs return over the tables of t (entries from user_fctx)."""
    rf.load_into_ref(r, t)
    qs, out = t["queries"], {}
    out["pq_search"] = np.stack([r.pq_search(q, K_LIST)[0] for q in qs])
    out["pq_search_in"] = np.stack([r.pq_search_in(q, K_LIST, t["subset"])[0] for q in qs])
    gi, gg, gs, _ = r.grouping_pq(t["subset"], t["group_ids"])
    assert gs.tolist() == t["group_ids"].tolist()
    out["grouping_ids"], out["grouping_group"] = gi, gg
    gi, gg, _, _ = r.grouping_pq(t["ids"], t["group_ids"])
    out["grouping_all_ids"], out["grouping_all_group"] = gi, gg
    for W in (1, 3, t["C"]):
        r.set_w(W) if W == 1 else (rf.load_into_ref(r, t, W=W))
        assert all(rf.rounds_without_cell_minus_one(t, q, K_LIST, W) for q in qs), "a query would reach the reference's cell -1"
        out[f"ivfadc_search_w{W}"] = np.stack([r.ivfadc_search(q, K_LIST)[0] for q in qs])
    qid, ent, _ = r.ivfadc_batch_search(t["query_ids"], K_LIST)
    out["batch_query_ids"], out["ivfadc_batch_search"] = qid, ent
    return out


def tables_from_file(z):
    """The stored arrays as the dict load_into_ref / oracle_tables want (the vectors table holds the fetched rows only)."""
    t = {k: z[k] for k in z.files}
    m, K, _ = t["codebook"].shape
    t.update(m=m, K=K, C=t["coarse"].shape[0], N=t["ids"].size, d=t["coarse"].shape[1], pq_codebook=t["codebook"])
    order = np.lexsort((t["ids"], t["cell"]))
    t["list_off"] = np.zeros(t["C"] + 1, np.int32)
    t["list_off"][1:] = np.cumsum(np.bincount(t["cell"], minlength=t["C"]))
    t["ivf_ids"], t["ivf_codes"] = t["ids"][order], t["codes"][order]
    t["entry_order"] = np.random.default_rng(1).permutation(m * K)
    t["x_rows"] = (t["vec_ids"], t["vecs"])                            # the vectors table: only the rows that are fetched
    return t


def main():
    o, r = Oracle(), Ref()
    for name, shape in SHAPES.items():
        t = build(o, **shape)
        out = {k: t[k] for k in STORED}
        out.update(reference_outputs(r, t))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        assert size <= 500 * 1000, "a fixture above 500 KB"


if __name__ == "__main__":
    main()
