"""Small indexes shared by the reference pins (tests/test_ref_pin_cpu.py) and tests/golden/make_ref_golden.py: built with
numpy and the oracle's encoders, loaded into the oracle's tables and into the in-memory SPI of the reference build."""
import numpy as np


def small_index(o, d, m, K, C, N, seed, dup=((70, 100, 30),)):
    """Normalised rows with exact duplicates (distance ties), a flat PQ index and an IVFADC index over them."""
    rng = np.random.default_rng(seed)
    s = d // m
    base = rng.standard_normal((40, d)).astype(np.float32)
    x = base[rng.integers(0, 40, N)] + 0.05 * rng.standard_normal((N, d)).astype(np.float32)
    for src, dst, n in dup:
        x[dst:dst + n] = x[src:src + n]
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    ids = np.arange(1, N + 1, dtype=np.int32)
    coarse = x[rng.choice(N, C, replace=False)].copy()
    codebook = (0.15 * rng.standard_normal((m, K, s))).astype(np.float32)
    pq_codebook = x[rng.choice(N, K, replace=(K > N))].reshape(K, m, s).transpose(1, 0, 2).copy()
    if K > N:
        pq_codebook += (0.01 * rng.standard_normal(pq_codebook.shape)).astype(np.float32)
    pq_codes = o.encode_pq(pq_codebook, x)
    cell = o.assign_coarse(coarse, x)
    res = (x - coarse[cell]).astype(np.float32)                      # one binary32 subtraction per element, as vec_minus
    codes = o.encode_pq(codebook, res)
    order = np.lexsort((ids, cell))
    list_off = np.zeros(C + 1, np.int32)
    list_off[1:] = np.cumsum(np.bincount(cell, minlength=C))
    return dict(d=d, m=m, K=K, C=C, N=N, x=x, ids=ids, coarse=coarse, codebook=codebook, pq_codebook=pq_codebook,
                pq_codes=pq_codes, cell=cell.astype(np.int32), codes=codes, list_off=list_off, ivf_ids=ids[order],
                ivf_codes=codes[order], entry_order=rng.permutation(m * K))


def oracle_tables(o, t):
    return (o.pq_table(t["pq_codebook"], t["ids"], t["pq_codes"]),
            o.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ivf_ids"], t["ivf_codes"]))


def load_into_ref(r, t, W=None):
    """Every table in ascending id (the stored order the oracle calls canonical); codebook tuples shuffled."""
    r.reset_tables()
    r.add_codebook("pq_codebook", t["pq_codebook"], t["entry_order"])
    r.add_codebook("residual_codebook", t["codebook"], t["entry_order"])
    r.add_pq_rows(t["ids"], t["pq_codes"])
    r.add_vectors("coarse_quantization", np.arange(t["C"]), t["coarse"])
    r.add_fine_rows(t["ids"], t["cell"], t["codes"])
    if "x_rows" in t:                                                  # (ids, vectors) of the only rows that are fetched
        r.add_vectors("vecs_norm", *t["x_rows"])
    else:
        r.add_vectors("vecs_norm", t["ids"], t["x"])
    if W is not None:
        r.set_w(W)


def rounds_without_cell_minus_one(t, q, k, W):
    """ivfadc_search probes W unused cells per round until it has fetched k rows.  With fewer than W cells left the
    reference selects cell -1 (undefined).  True when the search ends before that."""
    dist = ((t["coarse"].astype(np.float64) - q.astype(np.float64)) ** 2).sum(1)
    sizes = np.diff(t["list_off"])[np.argsort(dist, kind="stable")]
    for r in range(1, t["C"] // W + 1):
        if sizes[:r * W].sum() >= k:
            return True
    return False
