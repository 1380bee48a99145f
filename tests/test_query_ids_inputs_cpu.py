"""The inputs of tests/test_gpu_query_ids.py (tests/query_ids_inputs.py) reach what they claim, proven on the CPU."""
import numpy as np
import pytest

import dev_contract_inputs as dci
import query_ids_inputs as qi


def test_vector_ids_are_not_serial_and_the_table_is_no_multiple_of_64():
    ids = qi.vec_ids(qi.NV)
    assert qi.NV % 64 != 0 and ids.size == qi.NV
    assert (np.diff(ids) == 3).all() and ids[0] == 1
    assert int(ids[-1]) - int(ids[0]) + 1 != ids.size          # (the test of a serial table: last - first + 1 == N)


@pytest.mark.parametrize("n", qi.COUNTS)
def test_id_arrays_hold_every_kind_of_id(n):
    ids = qi.vec_ids(qi.NV)
    known = qi.known_ids(ids, n, seed=n)
    assert known.size == n and np.unique(known).size == n and np.isin(known, ids).all()
    if n >= 2:
        assert ids[0] in known and ids[-1] in known                # row 0 and row N - 1
    if n >= 3:
        assert (np.diff(known) < 0).any()                          # not in table order
    noisy = qi.noisy_ids(ids, known, seed=n)
    have = np.isin(noisy, ids)
    assert np.unique(noisy[have]).size < have.sum()                # duplicates
    assert (noisy < ids[0]).any() and (noisy > ids[-1]).any()      # below the smallest id, above the largest
    gap = noisy[~have & (noisy > ids[0]) & (noisy < ids[-1])]
    assert gap.size >= 1                                           # inside a gap
    assert not have[0] and not have[-1] and (~have[1:-1]).any()    # unknown ids in the first, a middle and the last slot
    # the model: TABLE_ORDER = the distinct known ids ascending; POSITIONAL = the array, -1 rows where there is none
    sel, rows = qi.model(ids, noisy, qi.TABLE_ORDER)
    assert sel.tolist() == sorted(set(known.tolist())) and (ids[rows] == sel).all()
    sel, rows = qi.model(ids, noisy, qi.POSITIONAL)
    assert np.array_equal(sel, noisy) and np.array_equal(rows >= 0, have) and (ids[rows[have]] == noisy[have]).all()


def test_vector_tables_differ_from_the_ann_tables():
    for shape in qi.SHAPES:
        c = qi.case(shape)
        ann = np.sort(c["ivf"]["ids"])
        assert c["vec_x"].shape == (qi.NV, c["ivf"]["coarse"].shape[1])
        assert (~np.isin(c["vec_ids"], ann)).any() or c["vec_ids"][-1] <= ann[-1]
        assert (~np.isin(ann, c["vec_ids"])).any()                 # ids the ANN table has and the vector table lacks
    c = qi.case("d300_k256")
    x = qi.pm.main_tables()[0]
    tail = c["vec_x"][-999:]
    assert not (tail[:, None, :5] == x[None, :200, :5]).all(-1).any()    # (a spot check: the negated rows are no corpus rows)
    assert c["vec_x"].shape[1] * 4 % 16 == 0 and c["vec_x"].shape[1] // 4 == 75
    assert qi.case("d25")["vec_x"].shape[1] % 4 != 0 and qi.case("d8")["vec_x"].shape[1] // 4 == 2


@pytest.mark.parametrize("W,rule,sentinel", qi.straggler_runs())
def test_straggler_batch_has_finished_and_unfinished_queries(W, rule, sentinel):
    """Round one (max_rounds = 1) leaves queries with found < k next to finished ones, in the batch as a whole and inside one of the
    sub-batches that option pipeline_batch = 64 cuts it into; the uncapped search probes again for exactly those."""
    s = qi.straggler_case(W)
    c, qs, k = s["c"], s["vec_x"], qi.STRAGGLER_KEY[2]
    one, found, _ = dci.search(c, qs, k, W, rule, 1, sentinel=sentinel)
    full, found_full, rounds = dci.search(c, qs, k, W, rule, 0, sentinel=sentinel)
    un = found < k
    assert un.any() and (~un).any()
    per = -(-qs.shape[0] // -(-qs.shape[0] // 64))                 # the equal sub-batches of option pipeline_batch = 64
    mixed = [un[a:a + per].any() and (~un[a:a + per]).any() for a in range(0, qs.shape[0], per)]
    assert any(mixed), "no sub-batch holds both kinds"
    assert (rounds[un] > 1).all() and (rounds[~un] == 1).all()     # the full search probes again for exactly those
