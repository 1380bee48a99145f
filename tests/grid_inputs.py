"""The grids and path choices made from the handle's CU count (postgres-word2vec_amd/csrc/grid_plan.h), restated twice: PARENT, the
expressions as the .hip files spelled them before the header existed, and PLAN, as the header has them; and CASES, the GPU cases of
tests/test_gpu_grid_cus.py with their sizes.  tests/test_grid_inputs_cpu.py compares the compiled header with both restatements and
proves for every case that at its grid_cus values the grid is smaller than the work by the stated factor -- so that a case whose
loop would not iterate fails on the CPU.

A function takes (n_cus, *work sizes and options) in the order the test program reads them from stdin and returns one integer."""
import functools

import numpy as np

DEVICE_CUS = 256                 # the chip the GPU suite runs on
GRID_CUS = (1, 2, 3, 7)          # what every GPU case runs at unless it says otherwise
SWEEP_CUS = (1, 2, 3, 7, 32, 256, 304)
# csrc constants the formulas are called with
SCAN5_G, SPEC2_G, MULTI_G = 16, 12, 8      # items per work entry: fused5.h / fused8.h, fused3.h, multi.h
ONE_WAVES, ONE_M = 8, 12                    # one_layout.h
AS_PQ_WG, SIM_AT = 256, 16                  # assign.h: AS_PQ_WG; dot_chain.h: TILE_QT, the A rows per tile of sim_matrix_kernel
EXF_WAVES = 8                               # exact2.h: EXF_WG / 64


def _cdiv(a, b):
    return -(-a // b)


# ---- PARENT: as ivfadc.hip, pq.hip, exact.hip and exact_host.h had them ------------------------------------------------------------
def _p_scan_cus(n, share, reserve):
    return max(n // max(1, share), min(n, 32)) - reserve


PARENT = {
    "grid_cus": lambda v, dev: dev if v <= 0 else min(v, dev),      # (new with the option: as include/freddy_gpu.h states it)
    "own": lambda n, share, reserve, mg: min(mg, max(1, _p_scan_cus(n, share, reserve))),
    "cap": lambda n, el_reserve, reserve, share: n - el_reserve - reserve * share,
    "persist": lambda elastic, n_own, cap, mg: min(mg, max(n_own, cap)) if elastic else n_own,
    "sparse_grid": lambda n, share, reserve, sp_cap, pairs: min(sp_cap, max(1, _p_scan_cus(n, share, reserve)) * (3 if pairs else 6)),
    "sparse_rule": lambda n, n_items, C: int(n_items < 4 * C and n_items >= 16 * n),
    "spec2": lambda n, mg: min(mg, n),
    "multi": lambda n, mg, lds: min(mg, n * max(1, min(2, (150 * 1024) // lds))),
    "ivf_one": lambda n, L: max(1, min(n, 256, (56 * 1024) // (8 * L))),
    "pq_one": lambda n, L, n_blocks, waves: max(1, min(n, 256, (n_blocks + waves - 1) // waves, (56 * 1024) // (8 * L))),
    "rpt": lambda n, targets, wg: 4 if targets >= n * 2 * 4 * wg else 1,
    "filter_grid": lambda n, rows: max(1, min((rows + 255) // 256, n * 2)),
    "join_gx": lambda n, rows, qtiles: max(1, min((rows + 255) // 256, max(n * 2 // qtiles, ((rows + 255) // 256 + 7) // 8))),
    "stats": lambda n, rows: min((rows + 3) // 4, n * 8),
    "sim_split": lambda n, n_tiles, nblk: min(n_tiles, max(1, (16 * n + nblk - 1) // nblk)),
    "sim_tiles": lambda n, n_tiles, nblk: _cdiv(n_tiles, min(n_tiles, max(1, (16 * n + nblk - 1) // nblk))),
    "sim_grid_y": lambda n, n_tiles, nblk: _cdiv(n_tiles, _cdiv(n_tiles, min(n_tiles, max(1, (16 * n + nblk - 1) // nblk)))),
}


# ---- PLAN: as grid_plan.h has them (numpy, element-wise) ----------------------------------------------------------------------------
def _scan_cus(n, share, reserve):
    return np.maximum(n // np.maximum(1, share), np.minimum(n, 32)) - reserve


def _sim_split(n, n_tiles, nblk):
    return np.minimum(n_tiles, np.maximum(1, (16 * n + nblk - 1) // nblk))


def _sim_tiles(n, n_tiles, nblk):
    s = _sim_split(n, n_tiles, nblk)
    return (n_tiles + s - 1) // s


def _join_gx(n, rows, qtiles):
    steps = (rows + 255) // 256
    return np.maximum(1, np.minimum(steps, np.maximum(n * 2 // qtiles, (steps + 7) // 8)))


PLAN = {
    "grid_cus": lambda v, dev: np.where(v <= 0, dev, np.minimum(v, dev)),
    "own": lambda n, share, reserve, mg: np.minimum(mg, np.maximum(1, _scan_cus(n, share, reserve))),
    "cap": lambda n, el_reserve, reserve, share: n - el_reserve - reserve * share,
    "persist": lambda elastic, n_own, cap, mg: np.where(elastic != 0, np.minimum(mg, np.maximum(n_own, cap)), n_own),
    "sparse_grid": lambda n, share, reserve, sp_cap, pairs: np.minimum(sp_cap, np.maximum(1, _scan_cus(n, share, reserve)) * np.where(pairs != 0, 3, 6)),
    "sparse_rule": lambda n, n_items, C: ((n_items < 4 * C) & (n_items >= 16 * n)).astype(np.int64),
    "spec2": lambda n, mg: np.minimum(mg, n),
    "multi": lambda n, mg, lds: np.minimum(mg, n * np.maximum(1, np.minimum(2, (150 * 1024) // lds))),
    "ivf_one": lambda n, L: np.maximum(1, np.minimum(np.minimum(n, 256), (56 * 1024) // (8 * L))),
    "pq_one": lambda n, L, n_blocks, waves: np.maximum(1, np.minimum(np.minimum(n, 256), np.minimum((n_blocks + waves - 1) // waves, (56 * 1024) // (8 * L)))),
    "rpt": lambda n, targets, wg: np.where(targets >= n * 2 * 4 * wg, 4, 1),
    "filter_grid": lambda n, rows: np.maximum(1, np.minimum((rows + 255) // 256, n * 2)),
    "join_gx": _join_gx,
    "stats": lambda n, rows: np.minimum((rows + 3) // 4, n * 8),
    "sim_split": _sim_split,
    "sim_tiles": _sim_tiles,
    "sim_grid_y": lambda n, n_tiles, nblk: (n_tiles + _sim_tiles(n, n_tiles, nblk) - 1) // _sim_tiles(n, n_tiles, nblk),
}


def plan(fn, *args):
    return int(PLAN[fn](*[np.int64(a) for a in args]))


# ---- work sizes ------------------------------------------------------------------------------------------------------------------
def max_groups(n_items, C, upi=1):
    """ivf_work_table: the bound of the work entries of a round, whichever scan runs"""
    return (n_items // MULTI_G + C + 1) * upi


def multi_lds(m, K):
    """multi.h multi_lds_bytes"""
    return m * K * MULTI_G * 4 + MULTI_G * 64 * 4 + MULTI_G * 4 + 64


def ivf_one_lds(K, C, W, L, G):
    """one_layout.h OneLayout::lds_bytes for ivf_one_kernel"""
    up = lambda n, a: (n + a - 1) // a * a
    lut = 4 * ONE_M * K
    scan = max(up(lut, 16) + ONE_WAVES * 64 * 8, ONE_WAVES * 64 * 8 + 8 * G * L)
    return max((_cdiv(C, G) + 1) * 300 * 4, C * 4 + 64 + 64 * 8 + 64, scan)


# ---- the tables of the GPU cases (sizes only; tests/test_gpu_grid_cus.py builds them with tests/util.py) -------------------------
IVF = dict(N=20000, C=32, d=300, m=12, Q=64, W=3)                  # case a, c: util.ivf_tables(N, C, K), K = 1024 and 256
SPARSE = dict(N=6000, C=200, d=300, m=12, K=256, Q=16, W=3)        # case b
MULTI = {"25x5x256": dict(d=25, m=5, K=256, C=32, N=8000, Q=64, W=3), "300x30x32": dict(d=300, m=30, K=32, C=32, N=8000, Q=64, W=3)}   # case d
PQ = dict(N=20000, lists=5)                                        # case e: five pseudo-lists of 4096 rows
ONE_IVF = dict(N=20000, C=32, K=256, W=3)                          # case f
ONE_IVF_WIDE = dict(N=20000, C=4096, K=256, W=3)
ONE_PQ = dict(N=5000, K=256)
EXACT = dict(N=8192 + 40)                                          # cases g, h; case i has about as many targets
JOIN = dict(targets=8200)
STATS = dict(N0=600, append=500)                                   # case j
SIM = dict(na=200, nb=(200, 1100))                                 # case k
ASSIGN = dict(targets=2148)


@functools.lru_cache(maxsize=None)
def sparse_tables():
    import util
    from freddy_amd import index_build as ib
    s = SPARSE
    return ib.build_ivf_index(util.corpus(s["N"]), C=s["C"], m=s["m"], K=s["K"], train_size=5000, iters=3, seed=9)


@functools.lru_cache(maxsize=None)
def sparse_queries():
    import util
    return util.queries_from_corpus(SPARSE["N"], SPARSE["Q"], seed=13)[1]


def thin_units(coarse, qs, W, most=2):
    """cells that 1 .. `most` queries of the batch probe in the first round (a cell of two items is ONE unit of the pair kernel):
    the item-wise scan's units where no list is longer than 4096 rows.  (float64 distances: a tie in binary32 could move one cell)"""
    d2 = ((qs[:, None, :].astype(np.float64) - coarse[None].astype(np.float64)) ** 2).sum(-1)
    cells = np.argsort(d2, axis=1, kind="stable")[:, :W]
    cnt = np.bincount(cells.ravel(), minlength=coarse.shape[0])
    return int(((cnt >= 1) & (cnt <= most)).sum())


# ---- CASES: (name, formula, arguments behind n_cus, grid_cus values, work_min, factor, grid at 256) ---------------------------
# work_min is a number of pieces the launch has AT LEAST (proved by counting, never measured): items / items-per-entry for the
# scans (all items in one cell give the fewest entries), units, strips per wave-slot and so on; `per` is how many pieces one
# workgroup of the grid takes at a time (waves for the strip loops).  The CPU test asserts  work_min >= factor * grid * per  at every
# listed grid_cus, and that the grid at 256 is `at256`.
def _case(name, fn, args, work_min, factor, at256, cus=GRID_CUS, per=1):
    return dict(name=name, fn=fn, args=tuple(args), cus=tuple(cus), work_min=work_min, factor=factor, at256=at256, per=per)


def cases():
    a = IVF
    items = a["Q"] * a["W"]
    mg = max_groups(items, a["C"])
    out = [
        # a. the filter scan: n_own workgroups over >= items / 16 entries
        _case("a.filter", "own", (1, 0, mg), _cdiv(items, SCAN5_G), 1.5, mg),
        _case("a.filter share 4", "own", (4, 0, mg), _cdiv(items, SCAN5_G), 4, mg, cus=(3,)),
        _case("a.filter two streams", "own", (2, 0, mg), _cdiv(items, SCAN5_G), 1.5, mg),
        # b. the item-wise scan (work: tests/test_grid_inputs_cpu.py counts the thin cells of the table itself)
        _case("b.sparse", "sparse_grid", (1, 0, SPARSE["Q"] * SPARSE["W"], 1), None, 2, SPARSE["Q"] * SPARSE["W"], cus=(1, 2, 3)),
        # c. the reference-arithmetic scan
        _case("c.spec2", "spec2", (mg,), _cdiv(items, SPEC2_G), 2, mg),
    ]
    for key, s in MULTI.items():     # d. the multi scan
        it = s["Q"] * s["W"]
        out.append(_case("d.multi " + key, "multi", (max_groups(it, s["C"]), multi_lds(s["m"], s["K"])), _cdiv(it, MULTI_G), 1.5,
                         max_groups(it, s["C"])))
    for Q, cus in ((16, (1, 2, 3)), (64, GRID_CUS)):     # e. the flat PQ table: ceil(Q / 16) entries per pseudo-list, exactly
        n_entries = _cdiv(Q, SCAN5_G) * PQ["lists"]
        out.append(_case(f"e.pq Q={Q}", "own", (1, 0, n_entries), n_entries, 1.5, n_entries, cus=cus))
    for k in (5, 32):                # f. one launch: W * 12 table units dealt round G workgroups
        out.append(_case(f"f.ivf_one k={k}", "ivf_one", (2 * k,), ONE_IVF["W"] * ONE_M, 2.5, min(256, 7168 // (2 * k)), cus=(3, 7, 13)))
    blocks = _cdiv(ONE_PQ["N"], 64)
    out.append(_case("f.pq_one", "pq_one", (10, blocks, ONE_WAVES), ONE_M, 1.5, _cdiv(blocks, ONE_WAVES)))
    # g, h. the strip loops of exf_filter_kernel / an_filter_kernel: 8 waves per workgroup, a strip of 32 rows each
    strips = _cdiv(EXACT["N"], 32)
    out.append(_case("g.exact filter", "filter_grid", (EXACT["N"],), strips, 2, _cdiv(EXACT["N"], 256), per=EXF_WAVES))
    out.append(_case("g.exact filter, 16 strips per wave", "filter_grid", (EXACT["N"],), strips, 16, _cdiv(EXACT["N"], 256), cus=(1,), per=EXF_WAVES))
    # i. the exact join: steps of 256 targets dealt round gx workgroups (Q = 70: one tile of 128 or two of 64; Q = 200: two or four)
    steps = _cdiv(JOIN["targets"], 256)
    for qtiles in (1, 2, 4):
        out.append(_case(f"i.join qtiles={qtiles}", "join_gx", (JOIN["targets"], qtiles), steps, 2, steps))
    # j. the table statistics: four rows per workgroup and sweep
    out.append(_case("j.stats pin", "stats", (STATS["N0"],), STATS["N0"], 18, _cdiv(STATS["N0"], 4), cus=(1,), per=4))
    out.append(_case("j.stats append", "stats", (STATS["append"],), STATS["append"], 15, _cdiv(STATS["append"], 4), cus=(1,), per=4))
    # k. similarity: tiles of 16 A rows per workgroup (sim_tiles IS the loop count: at least 3 at grid_cus = 1, 1 at 256)
    return out


def sim_cases():
    """(na, nb, grid_cus, tiles_per_wg, ragged): the similarity kernel's ranges of A tiles"""
    out = []
    for nb in SIM["nb"]:
        n_tiles, nblk = _cdiv(SIM["na"], SIM_AT), _cdiv(nb, 64)
        for n in GRID_CUS + (DEVICE_CUS,):
            t = plan("sim_tiles", n, n_tiles, nblk)
            out.append((SIM["na"], nb, n, t, n_tiles % t != 0))
    return out
