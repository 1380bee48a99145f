"""The chunk sizes of the search calls (postgres-word2vec_amd/csrc/chunk_plan.h) restated in Python, the budgets that dial a wanted
chunk size, and the cases tests/test_gpu_chunks.py runs -- shared with tests/test_chunk_plan_cpu.py, which compares the restatement
with the header compiled on its own and asserts, per GPU case, the regime of the formula it reaches and the number of chunks it is
cut into.  Plain integers only: nothing here touches a table or a device.

A call of Q queries is cut into chunks of at most `per` queries (for_chunks, csrc/ivf_run.h): ceil(Q / per) chunks, the last one
Q - (chunks - 1) * per queries.  `per` comes from option lut_budget_mb (MB of workspace per call):
  ivf_per        freddy_gpu_ivfadc_search_dev, the stragglers' re-search of a host-buffer call, and the cap of its sub-batches
  pq_fused_per   the flat PQ table through the cell-grouped scan (pseudo-lists of 4096 rows)
  pq_per         the flat PQ table through the generic scan
The regimes of ivf_per (ivf_regime):
  special   the 300-d / m = 12 / S = 25 shape, 2k <= 64: max(LUTs, survivor regions); "special-lut" where the LUT term is the larger
  multi     every other shape: LUTs + survivor regions
  wide      2k > 64: a list of min(2k, 1024) keys per (item, chunk) beside the LUTs
  bigk      2k > 1024: and the selection passes' keys
  long      lists of more than 8 (special) / 32 units of 4096 rows: no survivor bytes, and no bucket cap
  bucket    the 256 MiB / (4 C) cap on the per-cell item buckets binds: tens of thousands of cells -- CPU test only"""

SURV_UNIT = 8 * 8 * 8 * 64          # bytes of the survivor regions of one 4096-row unit: 8 waves x 8 x 64 keys of 8 bytes
BUCKET = 256 << 20
DEFAULT_MB = 8192                   # internal.h Tuning::lut_budget_mb
AUTO_ITEMS = 256                    # ivfadc_begin: fused = -1 takes the cell-grouped scans from this many (query, cell) items on


def cdiv(a, b):
    return -(-a // b)


def units_per_item(max_list_blocks):
    return max(1, cdiv(max_list_blocks, 64))


def blocks_of(rows):
    """row blocks (64 rows) of a list of `rows` rows"""
    return cdiv(rows, 64)


def _ivf_terms(m, K, W, k, upi, special, max_list_blocks):
    lut = 4 * m * K * W
    if 2 * k > 64:
        lut += 8 * W * max(1, cdiv(max_list_blocks, 256)) * min(2 * k, 1024)
        if 2 * k > 1024:
            lut += 8 * cdiv(2 * k, 1024) * 1024
    surv = W * upi * SURV_UNIT if upi <= (8 if special else 32) else 0
    return lut, surv


def ivf_per(mb, m, K, W, k, upi, special, C, max_list_blocks):
    lut, surv = _ivf_terms(m, K, W, k, upi, special, max_list_blocks)
    per_query = max(lut, surv) if special else lut + surv
    n = (mb << 20) // max(per_query, 1)
    if surv:
        n = min(n, BUCKET // (4 * max(C, 1)))
    return max(1, min(n, 1 << 20))


def ivf_regime(mb, m, K, W, k, upi, special, C, max_list_blocks):
    """the set of names (module docstring) that describe how ivf_per(...) came about"""
    lut, surv = _ivf_terms(m, K, W, k, upi, special, max_list_blocks)
    per_query = max(lut, surv) if special else lut + surv
    names = set()
    if not surv:
        names.add("long")
    elif special:
        names.add("special-lut" if lut > surv else "special")
    else:
        names.add("multi")
    if 2 * k > 64:
        names.add("wide")
    if 2 * k > 1024:
        names.add("bigk")
    if surv and BUCKET // (4 * max(C, 1)) < (mb << 20) // max(per_query, 1):
        names.add("bucket")
    return names


def pq_fused_per(mb, n_blocks):
    lists = max(1, cdiv(n_blocks, 64))
    n = min((mb << 20) // (lists * SURV_UNIT), BUCKET // (4 * lists))
    return max(16, min(n, 1 << 16))


def pq_per(mb, m, K, n_blocks, k):
    per_query = 4 * m * K + 8 * max(1, cdiv(n_blocks, 64)) * min(2 * k, 1024)
    if 2 * k > 1024:
        per_query += 8 * cdiv(2 * k, 1024) * 1024
    return min(max((mb << 20) // per_query, 1), 1 << 20)


def cuts(Q, per):
    """the chunks [(q0, n)] of a call"""
    return [(q0, min(per, Q - q0)) for q0 in range(0, Q, per)]


def budget_for(want, fn, *args, top=1 << 14):
    """the smallest lut_budget_mb at which fn(mb, *args) is `want` queries (None: no budget gives that size)"""
    for mb in range(1, top):
        n = fn(mb, *args)
        if n == want:
            return mb
        if n > want:
            return None
    return None


def sub_batches(Q, per, pipeline_batch=2048):
    """the sub-batches of a host-buffer IVFADC call (stage_plan.h pipe_cuts): equal ones within the cap"""
    cap = max(1, min(per, pipeline_batch))
    n_sub = cdiv(Q, cap)
    return cuts(Q, cdiv(Q, n_sub))


# ---- the tables of tests/test_gpu_chunks.py as the formulas see them -------------------------------------------------------------------
# (m, K, C, special, rows of the longest list at most / at least): the GPU tests assert the bounds on the rows of the table they pin
IVF_TABLES = {
    "K256": dict(m=12, K=256, C=64, special=True, max_rows=(1, 4096)),         # dev_contract_inputs ("300", 256, k): one unit per item
    "K1024": dict(m=12, K=1024, C=64, special=True, max_rows=(1, 4096)),       # ("300", 1024, 5)
    "k600": dict(m=12, K=256, C=64, special=True, max_rows=(1, 4096)),         # ("300", 256, 600): 60 000 rows
    "multi": dict(m=5, K=256, C=32, special=False, max_rows=(1, 4096)),        # soak_inputs.SHAPES (25, 5, 256), 8000 rows
    "long": dict(m=12, K=256, C=64, special=True, max_rows=(32769, 36864)),    # one list of nine units: 40 000 rows
    "main": dict(m=12, K=256, C=32, special=True, max_rows=(1, 4096)),         # pv_model.main_tables(): 20 000 rows
    "thin": dict(m=12, K=64, C=150, special=True, max_rows=(1, 4096)),         # the 600-row table of test_gpu_pipeline.py
}


def ivf_args(table, W, k, max_rows=None):
    """the formula's arguments behind the budget for a call with W probes and lists of k on `table` (W already cut to C)"""
    t = IVF_TABLES[table]
    mlb = blocks_of(t["max_rows"][1] if max_rows is None else max_rows)
    return (t["m"], t["K"], W, k, units_per_item(mlb), t["special"], t["C"], mlb)


def _dev_matrix():
    """IVFADC, freddy_gpu_ivfadc_search_dev: chunk sizes c with a tail of one query and without, on the K = 256 table with W = 32
    (1 MiB per query: the chunk is lut_budget_mb queries)"""
    out = []
    for c in (1, 31, 32, 33, 64, 65):
        for Q in (3 * c + 1, 3 * c):
            out.append(dict(id=f"c{c}-Q{Q}", table="K256", W=32, k=5, per=c, Q=Q, regime={"special"}))
    return out


DEV_MATRIX = _dev_matrix()
# one call per further regime: (table, W, k, wanted chunk size, Q) -> >= 3 chunks, the last one shorter
DEV_REGIMES = [
    dict(id="lut-term-K1024", table="K1024", W=4, k=5, per=21, Q=64, regime={"special-lut"}),
    dict(id="multi-25x5x256", table="multi", W=3, k=5, per=18, Q=64, regime={"multi"}),
    dict(id="wide-k40", table="K256", W=4, k=40, per=40, Q=121, regime={"special", "wide"}),
    dict(id="bigk-k600", table="k600", W=4, k=600, per=16, Q=50, regime={"special", "wide", "bigk"}),
    dict(id="long-list", table="long", W=8, k=5, per=21, Q=64, regime={"long"}),
]
# the unfinished queries of dev_contract_inputs' mixed batch (Q = 300, W = 1) in a middle chunk
DEV_MIDDLE = dict(id="middle", table="K256", W=1, k=5, per=96, Q=300, regime={"special"})
# host-buffer IVFADC calls: the cap of the sub-batches
HOST_CALLS = [
    dict(id="cap1-Q9", table="K256", W=32, k=5, per=1, Q=9, regime={"special"}),
    dict(id="cap33-Q100", table="K256", W=32, k=5, per=33, Q=100, regime={"special"}),
]
# the stragglers' re-search (ivfadc_sync_search) on the thin table: W = 1, k = 10, 65 stragglers among 85 queries.  The chunk size that
# cuts the re-search is the one that caps the sub-batch the stragglers come from (same handle, W and k), so a sub-batch's stragglers
# always fit ONE chunk: the loop in ivfadc_sync_search cannot be made to run twice through the public entry points.  What a budget
# does reach: 32 KiB per query and at least 1 MB, so sub-batches of at most 32 -- three of 29, 29 and 27, each with its own
# stragglers, re-searched one sub-batch after the other on the handle's stream and workspace with their extra probing rounds
STRAGGLERS = dict(id="stragglers", table="thin", W=1, k=10, per=32, Q=85, stragglers=65, regime={"special"})

# the entry points layered on the host-buffer calls (search_pv, search_ids, search_texts, the approximate analogies, a two-device
# handle) on pv_model.main_tables(): W = 3 and lists of at most 32 -- 96 KiB per query, sub-batches of at most 21; the flat table of
# 20 000 rows (313 row blocks, five pseudo-lists) in chunks of 32
LAYERS_IVF = dict(id="layers-ivf", table="main", W=3, k=30, per=21, Q=70, regime={"special"})
LAYERS_PQ = dict(id="layers-pq", N=20000, fused=1, k=30, per=32, Q=70)

# flat PQ: (rows, path, k, wanted chunk size, Q)
PQ_CALLS = [
    dict(id="fused-16-Q33", N=40000, fused=1, k=5, per=16, Q=33),
    dict(id="fused-16-Q48", N=40000, fused=1, k=5, per=16, Q=48),
    dict(id="fused-16-Q130", N=40000, fused=1, k=32, per=16, Q=130),
    dict(id="fused-19-Q58", N=40000, fused=1, k=5, per=19, Q=58),
    dict(id="fused-16-N4097-Q33", N=4097, fused=1, k=5, per=16, Q=33),
    dict(id="fused-48-N4097-Q130", N=4097, fused=1, k=1, per=48, Q=130),
    dict(id="generic-k32-Q121", N=40000, fused=0, k=32, per=60, Q=121),
    dict(id="generic-k600-Q55", N=40000, fused=0, k=600, per=18, Q=55),
    dict(id="generic-k5-N4097-Q169", N=4097, fused=0, k=5, per=84, Q=169),
    dict(id="generic-k600-N4097-Q47", N=4097, fused=0, k=600, per=23, Q=47),
]
# a subset of 5000 known ids of the 40 000-row table: 79 row blocks, two pseudo-lists -- the table's own 625 blocks give other sizes
PQ_SUBSET_ROWS = 5000
PQ_SUBSETS = [
    dict(id="subset-fused", N=40000, fused=1, k=5, per=32, Q=65),
    dict(id="subset-generic", N=40000, fused=0, k=5, per=84, Q=241),
]
PQ_M, PQ_K = 12, 256


def pq_budget(case, n_blocks):
    if case["fused"]:
        return budget_for(case["per"], pq_fused_per, n_blocks)
    return budget_for(case["per"], pq_per, PQ_M, PQ_K, n_blocks, case["k"])


def ivf_budget(case, max_rows=None):
    return budget_for(case["per"], ivf_per, *ivf_args(case["table"], case["W"], case["k"], max_rows))
