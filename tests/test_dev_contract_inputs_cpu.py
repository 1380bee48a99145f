"""CPU check of tests/dev_contract_inputs.py: the conditions under which tests/test_gpu_dev_contract.py is not vacuous.  A "none"
batch with an unfinished query, an "all" batch with a finished one or a "mixed" batch that is nearly one or the other would
let a status word that is never (or always) set pass; so would a sentinel cell whose query both found rules treat alike.  The
capped oracle alone; nothing here needs a device."""
import numpy as np
import pytest

import dev_contract_inputs as dci

CASES = list(dci.CASES)
CASES_W = [c + (W,) for c, Ws in dci.CASES.items() for W in Ws]


@pytest.mark.parametrize("shape,K,k,ties", CASES)
def test_thinned_cells_are_what_they_claim(shape, K, k, ties):
    c = dci.case(shape, K, k, ties)
    n = np.diff(c["list_off"])
    cells = c["cells"]
    assert (n[cells["E"]], n[cells["O"]], n[cells["M"]], n[cells["X"]], n[cells["S"]]) == (0, 1, k - 1, k, k)
    assert len(set(c["G"]) | set(cells.values())) == dci.N_GROUP + 5, "the thinned cells overlap"
    assert all(n[g] == (k - 1) // dci.N_GROUP for g in c["G"]) and n[c["G"]].sum() < k
    assert n.sum() == c["ids"].size == c["codes"].shape[0] <= 60000
    for a in range(len(n)):    # the library's precondition: ids ascending inside every list, unique overall
        assert (np.diff(c["ids"][c["list_off"][a]:c["list_off"][a + 1]]) > 0).all()
    assert np.unique(c["ids"]).size == c["ids"].size
    if ties:    # every list of at least two rows holds two rows of equal codes
        for a in range(len(n)):
            lo = c["list_off"][a]
            assert n[a] < 2 or (c["codes"][lo:lo + n[a]][:-1] == c["codes"][lo:lo + n[a]][1:]).all(1).any()


@pytest.mark.parametrize("shape,K,k,ties,W", CASES_W)
def test_batches_hold_the_unfinished_sets_they_claim(shape, K, k, ties, W):
    c = dci.case(shape, K, k, ties)
    b = dci.batches(shape, K, k, ties, W)
    assert b["none"][0].shape[0] == dci.Q_NONE and b["mixed"][0].shape[0] == dci.Q_MIXED and 8 <= b["all"][0].shape[0] <= 300
    by_design = {1: {"E", "O", "M"} | {f"G{j}" for j in range(8)}, 4: {f"G{j}" for j in range(8)}}[W]
    assert by_design <= set(b["all"][1]), "a query that is unfinished by design is missing from the `all` batch"
    assert "X" in b["none"][1], "the query of the cell of exactly k rows is not finished under every rule"
    for rule in dci.RULES[W]:
        none, mixed, every = (dci.expected(shape, K, k, ties, W, rule, name) for name in dci.BATCHES)
        assert none["unfinished"].sum() == 0
        assert every["unfinished"].all()
        assert mixed["unfinished"].sum() >= 5 and (~mixed["unfinished"]).sum() >= 5
        names = np.array(b["mixed"][1])
        assert mixed["unfinished"][np.isin(names, sorted(by_design))].all()
        # an unfinished query goes on: the uncapped oracle ran further rounds for it (unless no cell was left), a finished one did not
        assert (none["rounds"] == 1).all() and (every["rounds"] > 1).all()
        fin = ~mixed["unfinished"]
        assert np.array_equal(mixed["round_one"][fin], mixed["final"][fin])
    if W == 1:
        s = b["mixed"][1].index("S")
        rows, accepted = (dci.expected(shape, K, k, ties, 1, rule, "mixed") for rule in (0, 1))
        assert not rows["unfinished"][s] and accepted["unfinished"][s], "the sentinel cell does not tell the found rules apart"
        lst = rows["round_one"][s]
        assert (lst["id"] >= 0).sum() == k - 1 and lst["dist"][k - 1] == np.float32(c["sentinel"]), "k - 1 rows below the sentinel, one on it"


def test_rule_two_is_the_accepted_rule_at_one_probe():
    """ivfadc_batch_search (what the tests compare FREDDY_FOUND_BATCH_UDF with) and the per-query restatement agree round by round."""
    c = dci.case("300", 256, 5, False)
    qs, _ = dci.batches("300", 256, 5, False, 1)["mixed"]
    for cap in (1, 2, 0):
        a = dci.search(c, qs, 5, 1, 2, cap)
        b = dci.search(c, qs, 5, 1, 1, cap, sentinel=100.0)
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), cap


def test_which_unfinished_queries_hold_equal_distances():
    """merge_replay_kernel writes the word in two places: where no two of a query's candidates are equally far, and in the replay
    that equal distances need.  On the `ties` table the cell of k - 1 rows is the second kind, the empty cell and the cells of
    one row are the first; on the plain table all of them are the first."""
    for ties in (False, True):
        c = dci.case("300", 256, 5, ties)
        names = ["E", "O", "M"] + [f"G{j}" for j in range(8)]
        one, found, _ = dci.search(c, np.stack([c["designed"][n] for n in names]), 5, 1, 0, 1)
        assert (found < 5).all()
        for n, lst in zip(names, one):
            d = lst["dist"][lst["id"] >= 0]
            assert (np.unique(d).size < d.size) == (ties and n == "M"), (ties, n, d)
