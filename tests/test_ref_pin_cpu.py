"""The CPU oracle pinned to the reference's own C code.

oracle/_ref/libfreddy_ref.so holds the reference's C files, compiled unchanged against stand-in PostgreSQL headers.
Here every oracle function runs beside the reference function it restates, and every search SRF beside the oracle's
driver of the same name over the same tables (through an in-memory SPI).  Equality is bit for bit: floats as uint32
views, ids / ranks / counts exact.  No tolerances.

Three undefined behaviours of the reference are defined in the oracle (the tk[k] write of an unguarded updateTopK,
cell -1 when fewer than W cells are left, int16 overflow of pair codes) and a fourth case is a deliberate difference
(ivfadc_batch_search with every cell used re-scans its last cell: duplicates, or no end; the oracle retires the query).
The reference is never fed such inputs: each exclusion is a named filter below and every test asserts that at least
99 % of its generated cases were compared.

With the reference tree present a library that cannot be built or loaded FAILS these tests; they skip only where
neither the tree nor oracle/_ref exists."""
import numpy as np
import pytest

import ref_fixture as rf
from oracle import ref as R
from oracle.oracle import ENTRY

f32 = np.float32


@pytest.fixture(scope="module")
def ref():
    if R.status() == "absent":
        pytest.skip("neither the reference tree nor oracle/_ref exists")
    return R.Ref()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_entries(a, b, what=""):
    assert np.array_equal(a["id"], b["id"]), (what, a["id"], b["id"])
    assert np.array_equal(bits(a["dist"]), bits(b["dist"])), (what, a["dist"], b["dist"])


class Tally:
    """cases generated / compared: a filter that drops more than 1 % fails the test"""

    def __init__(self):
        self.generated = self.compared = 0

    def keep(self, ok):
        self.generated += 1
        self.compared += bool(ok)
        return bool(ok)

    def check(self):
        assert self.generated > 0 and self.compared >= 0.99 * self.generated, (self.compared, self.generated)


# ---- named filters on generated inputs ---------------------------------------------------------------------------
# (The tk[k] write of updateTopK needs no filter: it happens only when the distance is not below the last entry, and the
# drivers feed every stream through the call sites' guard `distance < maxDist`, as the oracle's fo_offer does.  The tests
# without a filter compare every generated case; their tally only counts.)
def filter_pair_code_fits_int16(K):
    """A pair code c0 + K*c1 is stored as int16 by the reference: K*K - 1 must not exceed 32767."""
    return K * K - 1 <= 32767


def filter_no_cell_minus_one(t, q, k, W):
    """ivfadc_search selects cell -1 once fewer than W unused cells are left (see ref_fixture)."""
    return rf.rounds_without_cell_minus_one(t, q, k, W)


def filter_batch_cells_not_exhausted(t, k):
    """ivfadc_batch_search ends only when every query accepted k rows; with k above the row count it re-scans the last cell."""
    return k <= t["N"]


def filter_nearest_exists(min_dist):
    """updateCodebook / grouping_pq leave the nearest entry uninitialised when nothing is nearer than 100."""
    return bool(np.all(min_dist < 100))


# ---- squareDistance ------------------------------------------------------------------------------------------------
def test_pin_sqdist(ref, oracle):
    t = Tally()
    rng = np.random.default_rng(1)
    cases = [([1, 2, 3], [0, 0, 0]), ([], []), ([1 + 2.0 ** -12], [0])]
    for n in (1, 5, 25, 300, 301):
        for scale in (1.0, 1e-3, 1e3, 1e-20, 1e-30):
            cases.append(((rng.standard_normal(n) * scale).astype(f32), (rng.standard_normal(n) * scale).astype(f32)))
    fused_differs = 0
    for _ in range(400):                                           # test_sqdist_is_not_fused's inputs
        a, b = rng.standard_normal(25).astype(f32), rng.standard_normal(25).astype(f32)
        acc = f32(0)
        for x, y in zip(a, b):
            d = f32(x - y)
            acc = f32(np.float64(acc) + np.float64(d) * np.float64(d))
        fused_differs += bits(acc)[0] != bits(oracle.sqdist(a, b))[0]
        cases.append((a, b))
    assert fused_differs > 20
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, np.inf, -np.inf, np.nan, 3e38, -3e38, 1.0], f32)
    for _ in range(200):
        n = int(rng.choice([1, 5, 25]))
        cases.append((rng.choice(specials, n), rng.choice(specials, n)))
    with np.errstate(all="ignore"):
        for a, b in cases:
            t.keep(True)
            got, exp = oracle.sqdist(a, b), ref.sqdist(a, b)
            assert bits(got)[0] == bits(exp)[0], (a, b, got, exp)       # NaN sign and payload included
    t.check()


# ---- getPrecomputedDistances(Double) -------------------------------------------------------------------------------
@pytest.mark.parametrize("m,K,s", [(12, 16, 25), (5, 256, 5), (30, 32, 10)])
def test_pin_lut(ref, oracle, m, K, s):
    t = Tally()
    rng = np.random.default_rng(m * K)
    pos, code = np.divmod(np.arange(m * K), K)
    for rep in range(4):
        t.keep(True)
        cb = (rng.standard_normal((m, K, s)) * (0.15 if rep else 30.0)).astype(f32)
        q = rng.standard_normal(m * s).astype(f32)
        perm = rng.permutation(m * K)                              # the reference indexes by the entry's own pos / code
        exp = ref.lut_entries(q, m, K, pos[perm], code[perm], cb.reshape(m * K, s)[perm])
        assert np.array_equal(bits(oracle.lut(q, cb)), bits(exp))
        assert np.array_equal(bits(oracle.lut_entries(q, K, pos[perm], code[perm], cb.reshape(m * K, s)[perm])), bits(exp))
        # the pair table reads entry j + pos*K as "the j-th entry of pos": position-major, codes shuffled inside a position
        inner = np.concatenate([p * K + rng.permutation(K) for p in range(m)])
        exp2 = ref.lut_entries(q, m, K, pos[inner], code[inner], cb.reshape(m * K, s)[inner], double=True)
        assert np.array_equal(bits(oracle.lut_double(q, cb)), bits(exp2))
    t.check()


# ---- computePQDistanceInt16 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [5, 12, 30])
def test_pin_adc(ref, oracle, m):
    t = Tally()
    rng = np.random.default_rng(m)
    assert not filter_pair_code_fits_int16(256) and not filter_pair_code_fits_int16(182)
    # plain tables of K codes, and pair tables of K*K slots for the K whose pair codes fit (181 is the largest)
    for K, pair_of in ((16, None), (256, None), (128 * 128, 128), (181 * 181, 181)):
        for rep in range(12):
            if not t.keep(pair_of is None or filter_pair_code_fits_int16(pair_of)):
                continue
            lut = (rng.random(m * K) * (1000 if rep % 2 else 1)).astype(f32)
            codes = rng.integers(0, K, m).astype(np.int16)
            if rep == 0:
                codes[:] = 0
            if rep == 1:
                codes[:] = K - 1
            if rep == 2:
                codes[::2], codes[1::2] = 0, K - 1
            assert bits(oracle.adc(lut, codes, K))[0] == bits(ref.adc(lut, codes, K))[0]
    t.check()


# ---- updateTopK, initTopK(s), cmpTopKEntry ------------------------------------------------------------------------
def topk_streams(rng, k):
    yield [3, 1, 2, 1, 1, 0.5], [10, 11, 12, 13, 14, 15], 100.0     # tests/test_oracle.py's hand-derived cases
    yield [1, 1, 1, 1], [1, 2, 3, 4], 100.0
    yield [1, 1, 1, 0.5], [1, 2, 3, 4], 100.0
    yield [2.0], [7], 1000.0
    yield [100.0, 250.0, float("nan"), 99.5], [1, 2, 3, 4], 100.0
    for rep in range(60):
        n = int(rng.integers(0, 300))
        sentinel = [100.0, 1000.0, 100.5, 99.999][rep % 4]
        d = (rng.integers(0, 6, n) / f32(4)).astype(f32)            # far more than half of the distances are equal
        if rep % 3 == 0:                                             # the sentinel, (int)sentinel and their neighbours
            edge = np.array([sentinel, int(sentinel), np.nextafter(f32(sentinel), f32(0)), np.nextafter(f32(int(sentinel)), f32(0)),
                             np.nextafter(f32(sentinel), f32(1e9)), np.inf, np.nan, -0.0, 0.0], f32)
            d = np.where(rng.random(n) < 0.4, rng.choice(edge, n), d).astype(f32)
        ids = rng.integers(0, 8, n) if rep % 2 else rng.permutation(n)   # equal ids too
        yield d, ids.astype(np.int32), sentinel


@pytest.mark.parametrize("k", [1, 2, 5, 64])
def test_pin_topk_stream(ref, oracle, k):
    t = Tally()
    rng = np.random.default_rng(k)
    for i, (d, ids, sentinel) in enumerate(topk_streams(rng, k)):
        t.keep(True)
        same_entries(oracle.topk_stream(d, ids, k, sentinel), ref.topk_stream(d, ids, k, sentinel, init_many=bool(i % 2)), (k, i))
    t.check()
    for a, b in [(1, 2), (2, 1), (1, 1), (0.0, -0.0), (np.inf, 1), (np.nan, 1), (1, np.nan)]:
        exp = int(f32(a) > f32(b)) - int(f32(a) < f32(b))
        assert ref.cmp_entries(a, b) == exp and ref.cmp_entries(a, b, pv=True) == exp


# ---- updateTopKPV, initTopKPV(s), cmpTopKPVEntry, postverify ------------------------------------------------------
@pytest.mark.parametrize("k,pvf", [(1, 1), (5, 1), (1, 5), (10, 10), (25, 4)])
def test_pin_topkpv_and_postverify(ref, oracle, k, pvf):
    t = Tally()
    rng = np.random.default_rng(k * 100 + pvf)
    n, d = k * pvf, 25
    for i, (dd, ids, sentinel) in enumerate(topk_streams(rng, n)):
        t.keep(True)
        got, vec = ref.topkpv_stream(dd, ids, n, sentinel, init_many=bool(i % 2))
        exp = oracle.topk_stream(dd, ids, n, sentinel)               # the PV list is the same list with a vector per slot
        same_entries(exp, got, (n, i))
        for slot in range(n):                                        # and the vector travels with its entry
            if got["id"][slot] == -1 and vec[slot] == -1:
                continue
            assert ids[vec[slot]] == got["id"][slot] and bits(f32(dd[vec[slot]]))[0] == bits(got["dist"][slot])[0]
    for rep in range(30):
        t.keep(True)
        q = rng.standard_normal(d).astype(f32)
        pool = (q + rng.standard_normal((max(n // 3, 1), d)) * 0.3).astype(f32)
        cv = pool[rng.integers(0, pool.shape[0], n)]                 # duplicate candidate vectors: equal distances
        ci = rng.permutation(n).astype(np.int32) + 1
        ci[rng.random(n) < 0.2] = -1                                 # holes
        sentinel = 1000.0 if rep % 2 else 2.0                        # 2.0: some candidates are at or above the sentinel
        same_entries(oracle.postverify(q, k, ci, cv, sentinel), ref.postverify(q, k, pvf, ci, cv, sentinel), (k, pvf, rep))
    t.check()


# ---- push / pop, determineCoarseIdsMultiWithStatistics(Multi) -----------------------------------------------------
def multi_cases(rng):
    d, half = 300, 150
    for Kc in (2, 4, 8):
        cells = Kc * Kc
        for rep in range(6):
            cq = rng.standard_normal((2, Kc, half)).astype(f32)
            qs = rng.standard_normal((7, d)).astype(f32)
            if rep % 3 == 1:                                         # tied CELL distances from distinct side distances:
                cq[:] = 0                                            # side distances 1, 4, 9, ... on both sides, query 0
                for c in range(Kc):
                    cq[0, c, c], cq[1, c, c] = c + 1, c + 1
                qs[:] = 0
                qs[1:, 200:] = rng.integers(-2, 3, (6, 100))         # integer offsets keep every sum exact
            counts = rng.integers(0, 50, cells)
            counts[rng.integers(0, cells)] += 5
            total = int(counts.sum())
            stats = np.append(counts / total, total).astype(f32)
            yield Kc, cq, qs, stats, total


def test_pin_multi_index_select(ref, oracle):
    t = Tally()
    rng = np.random.default_rng(5)
    for Kc, cq, qs, stats, total in multi_cases(rng):
        cells = Kc * Kc
        dummy_cb = np.zeros((30, 2, 10), f32)
        ot = oracle.ivpq_table(dummy_cb, cq, np.arange(1, 3), np.zeros(2), np.zeros((2, 30)), None, stats)
        active = np.array([0, 2, 3, 6], np.int32)
        n_targets = max(total // 3, 1)
        # confidence 2.0: never reached, every cell in ascending distance; 0.8 / 0.3: a prefix; min target count reached
        # exactly: the smallest confidence at which one more cell is taken
        for conf, mtc in [(2.0, 5), (0.8, 5), (0.3, 1), (0.5, n_targets), (0.8, n_targets + 1)]:
            t.keep(True)
            got, glast = oracle.multi_index_select(ot, qs, active, n_targets, mtc, conf)
            exp, elast = ref.multi_index_select(cq, stats, qs, active, n_targets, mtc, conf)
            assert glast == elast, (Kc, conf, mtc)
            for a, b in zip(got, exp):
                assert a.tolist() == b.tolist(), (Kc, conf, mtc, a, b)
    t.check()


def test_pin_flat_cell_selection(ref, oracle):
    """determineCoarseIdsMultiWithStatistics (one flat coarse quantizer) has no oracle counterpart: the kNN-join of this project
    is the multi-index one.  Held to its own contract with pinned parts: cells in ascending squareDistance (fo_sqdist), taken
    while getConfidenceHyp (fo_confidence_hyp) of the binary32 running sum of their frequencies is below the confidence, all
    cells at most; lastIteration iff every active query took all cells.  Distinct distances: qsort's order of equal keys is
    not part of the contract."""
    t = Tally()
    rng = np.random.default_rng(6)
    for cells in (1, 5, 16):
        for rep in range(6):
            d = 30
            cq = rng.standard_normal((cells, d)).astype(f32)
            qs = rng.standard_normal((7, d)).astype(f32)
            counts = rng.integers(0, 50, cells) + (rep == 0)
            counts[rng.integers(0, cells)] += 5
            total = int(counts.sum())
            stats = np.append(counts / total, total).astype(f32)
            active = np.array([0, 2, 3, 6], np.int32)
            n_targets = max(total // 3, 1)
            for conf, mtc in [(2.0, 5), (0.8, 5), (0.3, 1), (0.5, n_targets), (0.8, n_targets + 1)]:
                dist = np.array([[oracle.sqdist(qs[a], c) for c in cq] for a in active])
                if not t.keep(all(np.unique(row).size == cells for row in dist)):
                    continue
                got, last = ref.multi_index_select(cq, stats, qs, active, n_targets, mtc, conf, multi=False)
                exp_last = True
                for row, cl in zip(dist, got):
                    order, prob, n = np.argsort(row, kind="stable"), f32(0), 0
                    while oracle.confidence_hyp(mtc, n_targets, prob, int(stats[cells])) < f32(conf) and n < cells:
                        prob = f32(prob + stats[order[n]])
                        n += 1
                    assert cl.tolist() == order[:n].tolist(), (cells, conf, mtc)
                    exp_last &= n == cells
                assert last == exp_last
    t.check()


# ---- getConfidenceBin, getConfidenceHyp ---------------------------------------------------------------------------
def test_pin_confidence(ref, oracle):
    t = Tally()
    grid = [(10, 5, 0.5, 100), (5, 100, 0.0, 1000), (15, 1000, 0.02, 3000000), (500, 100000, 0.004, 3000000),
            (25, 4000, 0.01, 20000), (5, 300, 0.05, 20000), (3, 100, 0.9, 20000), (500, 100000, 0.0049, 3000000)]
    grid += [(50, 10000, p, 1000000) for p in np.linspace(0.001, 0.02, 30)]
    rng = np.random.default_rng(7)
    grid += [(int(rng.integers(1, 500)), int(rng.integers(1, 100000)), float(rng.random() ** 3), int(rng.integers(2, 3000000)))
             for _ in range(300)]
    grid += [(5, 100, 1.0, 1000), (5, 100, 0.5, 100), (5, 5, 0.5, 100)]      # sig == 0: p = 1, stat_size == size
    for e, n, p, S in grid:
        t.keep(True)
        got, exp = oracle.confidence_hyp(e, n, p, S), ref.confidence(e, n, p, S)
        assert bits(got)[0] == bits(exp)[0], (e, n, p, S, got, exp)       # NaN sign and payload included
    t.check()
    # getConfidenceBin has no oracle counterpart (nothing calls it): held to its own formula, each step in the type C gives it
    # (int * float -> float; anything times a double constant -> double; libm's sqrt / erf, which math.* call)
    import math
    for e, n, p in [(15, 1000, 0.02), (5, 300, 0.05), (3, 100, 0.9), (1, 10, 0.5), (50, 10000, 0.004)] + \
                   [(int(rng.integers(1, 500)), int(rng.integers(1, 100000)), float(rng.random() ** 3)) for _ in range(100)]:
        pf = f32(p)
        np_ = f32(f32(n) * pf)
        mu = np_
        sig = f32(math.sqrt(float(np_) * (1.0 - float(pf))))
        exp = f32(1.0 - 0.5 * (1 + math.erf((e - 0.5 - float(mu)) / (float(sig) * math.sqrt(2)))))
        assert bits(ref.confidence(e, n, p, hyp=False))[0] == bits(exp)[0], (e, n, p)


# ---- updateCodebook ------------------------------------------------------------------------------------------------
def test_pin_update_codebook(ref, oracle):
    t = Tally()
    rng = np.random.default_rng(9)
    for rep in range(40):
        m, K, s = [(4, 8, 5), (12, 16, 25), (5, 4, 3)][rep % 3]
        cb = (0.5 * rng.standard_normal((m, K, s))).astype(f32)
        n = int(rng.integers(0, 12))
        vecs = (0.5 * rng.standard_normal((n, m * s))).astype(f32)
        counts = rng.integers(0, 3, m * K).astype(np.int32)        # counts 0 and 1 among them
        if rep % 4 == 0 and n >= 2:                                  # two vectors at equal distance from two centroids
            cb[0, 1] = cb[0, 0]
            cb[:, 2] = cb[:, 3]
            vecs[0, :s], vecs[1, :s] = cb[0, 0] + f32(0.25), cb[0, 0] + f32(0.25)
            vecs[1] = vecs[0]
        order = rng.permutation(m * K) if rep % 2 else np.arange(m * K)
        mind = np.array([[((vecs[i, p * s:(p + 1) * s].astype(np.float64) - cb[p]) ** 2).sum(1).min() for p in range(m)]
                         for i in range(n)])
        # a count that stays 0 divides by zero in the reference too (defined in IEEE arithmetic): kept
        if not t.keep(filter_nearest_exists(mind)):
            continue
        with np.errstate(all="ignore"):
            ecb, ecnt, ecodes, eincs = ref.update_codebook(cb, counts, vecs, order)
            gcb, gcnt, gcodes, gincs = oracle.update_codebook(cb, counts, vecs, order)
            assert np.array_equal(gcodes.astype(np.int32), ecodes) and np.array_equal(gincs, eincs)
            touched = eincs > 0                                      # only these are written back, through "%f" text
            exp_cb = np.where(touched[:, None], oracle.text_roundtrip(ecb.reshape(m * K, s)), cb.reshape(m * K, s))
        assert np.array_equal(bits(gcb.reshape(m * K, s)), bits(exp_cb)), rep
        assert np.array_equal(gcnt, np.where(touched, ecnt, counts)), rep
    t.check()


# ---- addToTargetList, inBlacklist / addToBlacklist ----------------------------------------------------------------
def test_pin_target_list_and_blacklist(ref):
    """The oracle has no function of its own here: ivpq_search_in walks a query's targets in arrival order, repeated ids
    included (fo_ivpq_search_in's target-list branch), and ivfadc_search skips cells by id.  Pinned: the chain keeps arrival
    order and every id, a list that fills exactly opens an empty one, and the blacklist is a set."""
    rng = np.random.default_rng(11)
    for method in (0, 1, 2):
        for size in (1, 2, 5):
            for n in (0, 1, size - 1, size, size + 1, 3 * size, 3 * size + 1):
                ids = rng.integers(0, 4, n).astype(np.int32)       # repeated ids
                got, sizes = ref.target_list(ids, size, method)
                assert got.tolist() == ids.tolist()
                assert sizes.tolist() == [size] * (n // size) + [n % size]     # filled exactly: a trailing empty list
    for rep in range(30):
        add = rng.integers(-1, 12, int(rng.integers(0, 10))).astype(np.int32)
        ask = np.arange(-2, 14, dtype=np.int32)
        assert ref.blacklist(add, ask).tolist() == np.isin(ask, add).tolist()


# ---- convert_bytea_* -----------------------------------------------------------------------------------------------
def test_pin_bytea_convert(ref, oracle):
    rng = np.random.default_rng(13)
    for dtype, width in ((np.float32, 4), (np.int32, 4), (np.int16, 2)):
        for n in (0, 1, 3, 25, 301):
            a = (rng.standard_normal(n) * 1000).astype(dtype)
            if dtype == np.float32 and n >= 3:
                a[:3] = [np.nan, -0.0, 1e-45]
            for pre in (False, True):
                if pre and n == 0:
                    continue                                         # size 0 means "allocate"
                back, varsize = ref.bytea_roundtrip(a, preallocated=pre)
                assert varsize == 4 + n * width
                assert back.tobytes() == a.tobytes()


# ---- cosine_similarity_simple(_norm), cosine_similarity_bytea ------------------------------------------------------
def test_pin_cosine_similarity(ref, oracle):
    rng = np.random.default_rng(15)
    cases = [(np.zeros(5, f32), rng.standard_normal(5).astype(f32)), (np.zeros(1, f32), np.zeros(1, f32))]
    for n in (1, 25, 300):
        for _ in range(10):
            cases.append((rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)))
    for a, b in cases:
        # binary64 chain in index order, as the reference writes it (the oracle's exact kNN uses the bytea form below)
        dot = na = nb = 0.0
        for x, y in zip(a.astype(np.float64), b.astype(np.float64)):
            dot += x * y
            nb += y * y
            na += x * x
        assert ref.cosine_simple(a, b, norm=True) == dot
        exp = dot / (np.sqrt(na) * np.sqrt(nb)) if na > 0 and nb > 0 else 0.0
        assert ref.cosine_simple(a, b) == exp
        if ref.have_core_functions():
            assert bits(oracle.cosine_similarity_bytea(a, b))[0] == bits(ref.cosine_similarity_bytea(a, b))[0]


# ---- core_functions.c: vec_minus / vec_plus / vec_normalize_bytea -------------------------------------------------
def test_pin_vec_ops(ref, oracle):
    assert ref.have_core_functions()        # core_functions.c compiles with the stand-ins
    rng = np.random.default_rng(17)
    with np.errstate(all="ignore"):
        for n in (1, 25, 300, 301):
            for scale in (1.0, 1e-20, 1e20):
                a, b = (rng.standard_normal(n) * scale).astype(f32), (rng.standard_normal(n) * scale).astype(f32)
                assert np.array_equal(bits(oracle.vec_minus(a, b)), bits(ref.vec_minus(a, b)))
                assert np.array_equal(bits(oracle.vec_plus(a, b)), bits(ref.vec_plus(a, b)))
                g, e = oracle.vec_normalize(a), ref.vec_normalize(a)
                assert np.array_equal(bits(g), bits(e)) or (np.isnan(g).all() and np.isnan(e).all())
        z = np.zeros(4, f32)                                         # the zero vector: 0 / 0
        assert np.isnan(oracle.vec_normalize(z)).all() and np.isnan(ref.vec_normalize(z)).all()


# ===================================================================================================================
# SRF level: the reference's set-returning functions over the in-memory SPI, beside the oracle's drivers
# ===================================================================================================================
SHAPES = {"d300": dict(d=300, m=12, K=16, C=8, N=360, seed=20260101),          # tests/golden/make_golden.py's
          "d25": dict(d=25, m=5, K=256, C=32, N=360, seed=20260102)}           # the reference's other shipped shape


@pytest.fixture(scope="module", params=sorted(SHAPES))
def index(request, oracle):
    t = rf.small_index(oracle, **SHAPES[request.param])
    t["pq_t"], t["ivf_t"] = rf.oracle_tables(oracle, t)
    rng = np.random.default_rng(3)
    inside = np.array([3, 71, 101, 250, 300, 359])                   # rows 71 and 101 are exact duplicates of each other
    outside = rng.standard_normal((2, t["d"])).astype(f32)
    outside /= np.linalg.norm(outside, axis=1, keepdims=True)
    t["queries"] = np.concatenate([t["x"][inside], outside.astype(f32)])
    t["query_rows"] = inside
    return t


def check_emitted(oracle, strs, entries, id_col=0):
    """the rows as text: "%d" of the id, "%f" of the distance -- against the oracle's emit path"""
    assert len(strs) == entries.size
    for row, e in zip(strs, entries.ravel()):
        assert int(row[id_col]) == int(e["id"]) and row[id_col] == "%d" % e["id"]
        assert row[id_col + 1] == "%f" % float(e["dist"])
        assert bits(f32(row[id_col + 1]))[0] == bits(oracle.emit_roundtrip(e["dist"]))[0]


def test_spi_stand_in(ref, oracle, index):
    """The in-memory SPI itself: stored order, IN as a set, ORDER BY, and an ERROR (never an empty result) for anything else."""
    rf.load_into_ref(ref, index, W=3)
    n, first = ref.spi("SELECT id, vector FROM pq_quantization")
    assert n == index["N"] and first.tolist() == index["ids"].tolist()
    n, first = ref.spi("SELECT id, vector FROM pq_quantization WHERE id IN (17, 5, 5, 9999, -4)")
    assert first.tolist() == [5, 17]
    n, first = ref.spi("SELECT id, vector, coarse_id FROM fine_quantization WHERE coarse_id IN(2,0)")
    assert first.tolist() == index["ids"][np.isin(index["cell"], [0, 2])].tolist()
    n, first = ref.spi("SELECT q.id, q.vector FROM pq_quantization AS q WHERE q.id IN (9, 3) ORDER BY id ASC")
    assert first.tolist() == [3, 9]
    n, first = ref.spi("SELECT * FROM get_w()")
    assert n == 1 and first.tolist() == [3]
    n, first = ref.spi("SELECT * FROM pq_codebook ORDER BY pos")
    assert n == index["m"] * index["K"]
    for bad in ("DELETE FROM pq_quantization", "SELECT id FROM nowhere", "SELECT nothing FROM pq_quantization",
                "SELECT id FROM pq_quantization WHERE id = 3", "SELECT id FROM pq_quantization LIMIT 3",
                "UPDATE pq_codebook SET (vector, count) = (1, 2)", "SELECT id FROM pq_quantization WHERE id IN ()"):
        with pytest.raises(R.RefError, match="SPI cannot run this statement"):
            ref.spi(bad)
    assert ref.spi("SELECT id FROM pq_quantization")[0] == index["N"]        # and the library goes on working


def test_pin_srf_pq_search(ref, oracle, index):
    t = Tally()
    rf.load_into_ref(ref, index)
    for k in (1, 5, index["N"] + 7):                                 # the last: more than the rows found, sentinel rows
        for q in index["queries"]:
            t.keep(True)
            got, strs = ref.pq_search(q, k)
            same_entries(oracle.pq_search(index["pq_t"], q, k), got, k)
            check_emitted(oracle, strs, got)
    t.check()


def test_pin_srf_pq_search_in(ref, oracle, index):
    t = Tally()
    rf.load_into_ref(ref, index)
    rng = np.random.default_rng(4)
    subsets = [np.array([5, 17, 17, 72, 102, 300, 361, -4], np.int32), index["ids"][::3], index["ids"][::-1],
               np.array([71, 101, 72, 102], np.int32), rng.integers(-5, 400, 50).astype(np.int32), np.array([9999], np.int32)]
    for k in (1, 5, 60):
        for sub in subsets:                                          # k above the rows found: 60 > 4, > 0
            for q in index["queries"][[0, 1, 2, 6]]:
                t.keep(True)
                got, strs = ref.pq_search_in(q, k, sub)
                same_entries(oracle.pq_search_in(index["pq_t"], q, k, sub), got, (k, sub[:5]))
                check_emitted(oracle, strs, got)
    t.check()


def test_pin_srf_ivfadc_search(ref, oracle, index):
    t = Tally()
    sizes = np.diff(index["list_off"])
    for W in (1, 3, index["C"]):
        rf.load_into_ref(ref, index, W=W)
        # k above the rows of the first round, so that further rounds run: the found rule and the refresh of maxDist.  The k
        # are chosen per W so that whole rounds of W cells can meet them (W = C has one round: k <= N).
        ks = [1, 5, int(sizes.max()) + 3, index["N"] // 3]
        ks += {1: [int(sizes.max()) + 1, index["N"]], 3: [int(np.sort(sizes)[-3:].sum()) + 1]}.get(W, [index["N"]])
        for k in ks:
            for q in index["queries"]:
                if not t.keep(filter_no_cell_minus_one(index, q, k, W)):
                    continue
                got, strs = ref.ivfadc_search(q, k)
                same_entries(oracle.ivfadc_search(index["ivf_t"], q, k, W, sentinel=1000.0, found_rule=0), got, (W, k))
                check_emitted(oracle, strs, got)
    t.check()


def test_pin_srf_ivfadc_batch_search(ref, oracle, index):
    t = Tally()
    rf.load_into_ref(ref, index)
    ids = index["ids"]
    sizes = np.diff(index["list_off"])
    batches = [ids[index["query_rows"]], np.array([72, 4, 4, 251, 9999, 102], np.int32), ids[:40], np.array([1], np.int32),
               np.array([102, 72], np.int32)]
    assert not filter_batch_cells_not_exhausted(index, index["N"] + 1)     # the excluded case itself: never generated below
    for k in (1, 5, int(sizes.max()) + 3, index["N"] // 2, index["N"]):
        for b in batches:
            if not t.keep(filter_batch_cells_not_exhausted(index, k)):
                continue
            qid, got, strs = ref.ivfadc_batch_search(b, k)
            fetched = np.array(sorted(set(b.tolist()) & set(ids.tolist())), np.int32)   # stored order, each id once
            assert qid.tolist() == fetched.tolist()
            exp = oracle.ivfadc_batch_search(index["ivf_t"], index["x"][fetched - 1], k)
            same_entries(exp, got, (k, b[:4]))
            assert [int(r[0]) for r in strs] == np.repeat(qid, k).tolist()
            check_emitted(oracle, strs, got, id_col=1)
            # the batch UDF is the W = 1 search with the "accepted insertions" found rule and sentinel 100
            many = oracle.ivfadc_search_many(index["ivf_t"], index["x"][fetched - 1], k, 1, sentinel=100.0, found_rule=1)
            same_entries(many, got, ("W=1 form", k))
    t.check()


def test_pin_srf_grouping_pq(ref, oracle, index):
    t = Tally()
    rf.load_into_ref(ref, index)
    ids = index["ids"]
    for groups in ([10, 200, 350], [350, 10, 200], [71, 101, 5], [7]):            # 71 / 101: two equal group vectors
        for inp in (ids[::5], np.array([5, 17, 17, 72, 102, 300, 361, -4], np.int32), ids[::-1][:50]):
            g = np.array(groups, np.int32)
            gs = np.sort(g)
            gv = index["x"][gs - 1]
            lut_min = np.array([oracle.lut(v, index["pq_codebook"]).reshape(index["m"], -1).min(1).sum() for v in gv])
            if not t.keep(filter_nearest_exists(lut_min)):
                continue
            oi, og, sg, strs = ref.grouping_pq(inp, g)
            ei, eg = oracle.grouping_pq(index["pq_t"], gv, inp)
            assert sg.tolist() == gs.tolist()
            assert oi.tolist() == ei.tolist() and og.tolist() == eg.tolist(), (groups, oi, ei, og, eg)
            assert [(int(a), int(b)) for a, b in strs] == [(int(i), int(gs[j])) for i, j in zip(ei, eg)]
    t.check()
    rf.load_into_ref(ref, index)
    with pytest.raises(R.RefError, match="Group ids do not exist"):              # an ERROR comes back as an exception
        ref.grouping_pq(ids[:5], np.array([10, 99999], np.int32))
