"""The inputs of tests/test_gpu_join_ids.py and tests/test_gpu_ivpq_analogy.py (tests/join_ids_inputs.py) are what the GPU tests rely on,
shown with the oracle alone: the query rows take every load path of sub_dist_rows_kernel, every shape runs a case for more than one
round, a query's list does not depend on the batch it is part of (which is what lets a positional call be checked slot by slot), and
the analogy's target sets produce what they are named for."""
import numpy as np
import pytest

import approx_analogy_model as am
import ivpq_analogy_model as im
import join_ids_inputs as ji
import util


def test_the_query_rows_take_every_load_path():
    rows = ji.query_rows()
    assert rows.size == ji.NQ and np.unique(rows).size == ji.NQ
    seen = set()
    for shape in ji.SHAPES:
        d = shape[0]
        x = np.asarray(ji.tables(shape)["vectors"], np.float32)
        assert x.shape == (ji.N, d) and np.array_equal(ji.tables(shape)["ids"], np.arange(1, ji.N + 1))
        assert np.array_equal(x[rows], util.shape_queries(ji.N, d, ji.NQ, seed=21))
        half = d // 2
        assert d % 2 == 0 and half <= 512
        off = np.array([[r * d + pos * half for pos in (0, 1)] for r in rows])
        wide = half % 4 == 0
        if wide:
            assert (off % 4 == 0).all()                   # 16-byte loads throughout
        seen.add((wide, bool((off[:, 0] % 4 == 0).all())))   # (the rows' own offsets: the second half of a 300-d row starts at float 150)
    assert seen == {(False, False), (True, True), (False, True)}, seen   # scalar + unaligned rows, 16-byte loads, scalar + aligned rows


def test_the_vector_tables_differ_from_the_ivpq_table():
    for shape in ji.SHAPES:
        ivpq_ids = ji.tables(shape)["ids"]
        ids, x = ji.vec_table(shape, "more")
        assert (np.diff(ids) > 0).all() and x.shape == (ids.size, shape[0]) and (~np.isin(ids, ivpq_ids)).sum() == 100
        ids, x = ji.vec_table(shape, "fewer")
        assert (np.diff(ids) > 0).all() and x.shape == (ids.size, shape[0])
        assert ids[-1] - ids[0] + 1 != ids.size                                   # not serial: the row is looked up
        assert 0 < np.isin(ji.query_ids(), ids).sum() < ji.NQ                    # some query ids have a row there, some have none
        for which in ("same", "more", "fewer"):
            ids, _ = ji.vec_table(shape, which)
            noisy = ji.noisy_positional(ji.query_ids())
            sel, rows = ji.model(ids, noisy, ji.POSITIONAL)
            assert (rows[[0, 3, 6, 8]] == -1).all() and noisy[0] < 0 and noisy[2] == noisy[4]   # unknown, negative and repeated ids


@pytest.mark.parametrize("shape", ji.SHAPES)
def test_rounds_and_independence(oracle, shape):
    """Every shape has a case that takes more than one round; for every case and method the lists of the sub-batch equal those rows of
    the whole batch's (the iteration counts need not: the contract names ONE call over the compacted batch)."""
    rows, most = ji.query_rows(), 0
    sub = rows[list(ji.SUB_BATCH)]
    for case in ji.CASES:
        for method in ji.METHODS:
            whole, it = ji.expected(oracle, shape, method, case)
            part, it_sub = ji.expected(oracle, shape, method, case, rows=sub)
            most = max(most, it)
            assert it_sub <= it
            w = whole[list(ji.SUB_BATCH)]
            assert np.array_equal(w["id"], part["id"]) and np.array_equal(w["dist"].view(np.uint32), part["dist"].view(np.uint32)), (shape, case, method)
            assert np.array_equal(part[1], part[2])                                                # the repeated query is answered again
    assert most > 1, (shape, most)
    k, _, _, T, _ = ji.CASES[3]
    whole, _ = ji.expected(oracle, shape, 0, ji.CASES[3])
    assert k == 60 and T == 3000 and (whole["id"] >= 0).all()                                       # full lists where targets abound


@pytest.fixture(scope="module")
def analogy(oracle):
    x, ids, t = ji.analogy_tables()
    return {"x": x, "ids": ids, "table": oracle.ivpq_table(*ji.pin_args(t)), "triples": am.main_triples()}


@pytest.mark.parametrize("method", ji.METHODS)
def test_the_analogy_target_sets_are_what_they_are_named_for(oracle, analogy, method):
    x, ids, table, triples = analogy["x"], analogy["ids"], analogy["table"], analogy["triples"]
    sets = ji.analogy_target_sets()
    base = ji.analogy_base()
    assert base.size == 4000 and not np.isin(base, triples[::2].reshape(-1)).any() and (~np.isin(base, ids)).sum() == 3

    def run(name, n_cand=4):
        tg, (alpha, pvf, conf) = sets[name]
        return im.expected(oracle, table, x, ids, triples, 1, n_cand, tg, alpha, pvf, method, confidence=conf)

    # all ids: some triples find an input among their candidates, so fewer are scored than there are candidates
    rows, stats, lists, raw, valid, iters = run("all")
    assert valid.all() and stats["searched"] == len(triples)
    with_input = sum(bool(np.isin(l[l >= 0], t).any()) for l, t in zip(lists, triples))
    assert with_input > 0 and stats["scored"] < stats["candidates"], (with_input, stats)
    # 300 targets at alpha = 1: more than one round
    rows, stats, lists, raw, valid, iters = run("base300")
    assert iters[0] > 1, iters
    # three targets, four slots: every list has fillers
    rows, stats, lists, raw, valid, iters = run("base3")
    assert ((lists < 0).sum(1) >= 1).all() and stats["candidates"] <= 3 * len(triples)
    # the three inputs of triple 7 as the only targets: its candidate set is empty
    rows, stats, lists, raw, valid, iters = run("inputs7")
    assert len(rows[7]) == 0 and np.isin(lists[7][lists[7] >= 0], triples[7]).all()
    # those and two more: more than one round
    rows, stats, lists, raw, valid, iters = run("inputs7+2")
    assert iters[0] > 1, iters
