"""The similarity model against the oracle, the float4 predicate against its table, and the reach of the case tables
(tests/similarity_inputs.py) -- all on the CPU."""
import numpy as np
import pytest

import similarity_inputs as si
import similarity_model as sm


def test_the_chain_is_the_oracles_cosine_similarity_bytea(oracle):
    rng = np.random.default_rng(1)
    n = 0
    for d in (300, 25, 32, 7, 1):
        a = rng.standard_normal((60, d)).astype(np.float32)
        b = rng.standard_normal((60, d)).astype(np.float32)
        a[40:50] *= np.float32(1e19); b[40:50] *= np.float32(1e19)          # products that overflow
        for r, val in ((50, np.inf), (51, -np.inf), (52, np.nan), (53, 0.0), (54, -0.0)):
            a[r, rng.integers(0, d)] = val
        b[55, :] = np.inf; a[55, :] = -1.0
        b[56, 0] = np.nan; b[57, d - 1] = -np.inf
        got = sm.chain(a, b)
        exp = np.array([oracle.cosine_similarity_bytea(a[i], b[i]) for i in range(60)], np.float32)
        assert sm.same_floats(got, exp), d
        assert np.array_equal(got[:40].view(np.uint32), exp[:40].view(np.uint32))
        n += 60
    assert n >= 300
    # broadcasting: a matrix is its pairs
    a, b = rng.standard_normal((5, 33)).astype(np.float32), rng.standard_normal((7, 33)).astype(np.float32)
    m = sm.chain(a[:, None, :], b[None, :, :])
    assert all(m[i, j].view(np.uint32) == oracle.cosine_similarity_bytea(a[i], b[j]).view(np.uint32) for i in range(5) for j in range(7))


def test_the_predicate_is_postgres_float4gt():
    for a, b, exp in sm.GT_CASES:
        assert bool(sm.float4gt(np.float32(a), np.float32(b))) is exp, (a, b, exp)
    # the order of the assign kernels separates the two zeros: it is not this predicate
    assert not sm.float4gt(np.float32(0.0), np.float32(-0.0))


def test_rows_of_and_the_three_calls_on_a_tiny_table(oracle):
    ids = np.array([3, 5, 6, 9], np.int32)
    x = np.arange(12, dtype=np.float32).reshape(4, 3) - 5
    assert sm.rows_of(ids, [3, 4, 9, 10, 2, 6]).tolist() == [0, -1, 3, -1, -1, 2]
    sim, known = sm.pairs(ids, x, [3, 4, 9], [9, 3, 9])
    assert known.tolist() == [True, False, True] and sim[1] == 0.0
    assert sim[0] == oracle.cosine_similarity_bytea(x[0], x[3]) and sim[2] == oracle.cosine_similarity_bytea(x[3], x[3])
    out, ka, kb = sm.matrix(ids, x, np.array([5, 7, 5]), [9, 8, 3])
    assert ka.tolist() == [True, False, True] and kb.tolist() == [True, False, True]
    assert out[1].tolist() == [0, 0, 0] and out[:, 1].tolist() == [0, 0, 0] and out[0, 0] == oracle.cosine_similarity_bytea(x[1], x[3])
    outv, kav, _ = sm.matrix(ids, x, x[[1, 0, 1]], [9, 8, 3])
    assert kav.all() and np.array_equal(outv[[0, 2]], out[[0, 2]])
    ia, ib, s, total = sm.join(ids, x, np.array([5, 7, 5]), [9, 8, 3], -100.0)
    assert (ia.tolist(), ib.tolist(), total) == ([0, 0, 2, 2], [0, 2, 0, 2], 4)        # unknown rows never match, i then j ascending
    ia, ib, s, total = sm.join(ids, x, np.array([5, 7, 5]), [9, 8, 3], -100.0, max_pairs=3)
    assert (ia.tolist(), ib.tolist(), total) == ([0, 0, 2], [0, 2, 0], 4)


def test_tables_have_gaps_and_every_kind_of_unknown_id():
    for d in si.DIMS:
        ids, x = si.table(d)
        assert x.shape == (si.TABLE_ROWS, d) and np.all(np.diff(ids) > 0) and (np.diff(ids) > 1).any()
        bad = si.unknown_ids(ids)
        assert (sm.rows_of(ids, bad) < 0).all() and bad.min() < ids[0] and bad.max() > ids[-1] and ((bad > ids[0]) & (bad < ids[-1])).any()
        assert len({r.tobytes() for r in x}) < len(x)                         # duplicate rows (ties)
    a, b = si.pair_case(300, 130)
    ra, rb = sm.rows_of(si.table(300)[0], a), sm.rows_of(si.table(300)[0], b)
    assert (ra < 0).any() and (rb < 0).any() and (a == b).any() and len(set(a.tolist())) < a.size
    a, b = si.matrix_case(300, 33, 200)
    ra, rb = sm.rows_of(si.table(300)[0], a), sm.rows_of(si.table(300)[0], b)
    assert (ra < 0).any() and (rb < 0).any() and np.intersect1d(a, b).size and len(set(b.tolist())) < b.size


@pytest.mark.parametrize("d", [12, 7])
def test_the_constructed_join_reaches_every_pattern(d):
    ids, x, a_ids, b_ids, thresholds = si.constructed(d)
    out, ka, kb = sm.matrix(ids, x, a_ids, b_ids)
    assert ka.tolist() == [True, True, True, False, True] and not kb[197] and kb.sum() == si.CON_NB - 1
    bits = out.view(np.uint32)
    thr = si.THR.view(np.uint32)
    # a similarity equal to the threshold bit for bit, its neighbour one ulp above
    assert bits[0, 192] == thr and bits[0, 193] == thr + 1
    assert np.isnan(out[0, 194]) and np.isnan(out[1, 194]) and np.isnan(out[2, 194])
    # +0.0 against the threshold -0.0
    z = np.delete(out[2], [194, 197])
    assert np.array_equal(z.view(np.uint32), np.zeros(z.size, np.uint32)) and np.signbit(thresholds[1]) and thresholds[1] == 0
    mask = ka[:, None] & kb[None, :] & sm.float4gt(out, si.THR)
    per_block = [mask[0, j:j + 64].sum() for j in range(0, si.CON_NB, 64)]
    assert per_block == [0, 1, 64, 2]
    assert mask[0, 127] and mask[0, 128] and not mask[0, 126]                 # the last lane of a block, then lane 0 of the next
    assert not mask[0, 192] and mask[0, 193] and mask[0, 194] and not mask[0, 195]
    assert mask[1].sum() == 2 and mask[1, 194] and mask[1, 195]
    assert not mask[3].any() and np.array_equal(mask[4], mask[0])
    ia, ib, s, total = sm.join_of(out, ka, kb, thresholds[1])                 # -0.0: the zero row matches only at its NaN
    assert ((ia == 2) & (ib != 194)).sum() == 0 and ((ia == 2) & (ib == 194)).sum() == 1
    assert sm.join_of(out, ka, kb, thresholds[2])[3] == 0                     # nothing is greater than a NaN threshold
    assert sm.join_of(out, ka, kb, thresholds[3])[3] == 4 * (si.CON_NB - 1)   # everything known is greater than -inf
    assert sm.join_of(out, ka, kb, thresholds[4])[3] == 4                     # only the NaNs are greater than +inf
    # the order: i ascending, then j ascending
    ia, ib, s, total = sm.join_of(out, ka, kb, si.THR)
    key = ia.astype(np.int64) * si.CON_NB + ib
    assert np.all(np.diff(key) > 0) and total == ia.size


def test_the_soak_and_the_poisoned_table():
    cases = si.soak_cases()
    assert len(cases) == 12 and {c[0] % 4 == 0 for c in cases} == {True, False} and {c[4] for c in cases} == {True, False}
    ids, x, rows = si.poisoned_table(300)
    assert np.isnan(x[rows]).any() and np.isinf(x[rows]).any()
    healthy = np.setdiff1d(np.arange(len(x)), rows)
    assert np.isfinite(x[healthy]).all()
    assert np.isneginf(sm.chain(x[1500], x[2998]))
