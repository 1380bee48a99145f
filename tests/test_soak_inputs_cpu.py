"""CPU check of tests/soak_inputs.py: a soak whose seeds never reach a regime tests nothing there.  Over exactly the seed lists
the GPU soaks parametrise over (soak_inputs.SEEDS), from the draws, the oracle and the numpy models alone, no regime below is
empty.  These are conditions, not measurements: another BASE or seed count is valid exactly when this file still passes.  Every
test prints the regimes with the seeds that reach them (pytest -s shows the table).

Every draw computes its expectations, so this file is also the suite's one full CPU run of them."""
import numpy as np
import pytest

import soak_inputs as si
import update_model as um


def _table(title, regimes):
    print(f"\n{title}")
    for name, seeds in regimes.items():
        print(f"  {name}: {seeds}")


def _none_empty(regimes):
    empty = [name for name, seeds in regimes.items() if not seeds]
    assert not empty, ("no seed reaches", empty)


def test_seed_lists():
    for family, seeds in si.SEEDS.items():
        assert family in si.BASE and len(seeds) >= 8 and len(set(seeds)) == len(seeds), family
    assert si.exj_min_targets() > 0 and si.exf_sample() > si.EXF_AUTO_ROWS and si.analogy_pass() == 32 and si.exf_pass() == 64


def test_draws_are_deterministic(oracle):
    a, b = si.draw_exact(si.SEEDS["exact"][0], oracle), si.draw_exact(si.SEEDS["exact"][0], oracle)
    assert a["label"] == b["label"] and np.array_equal(a["x"], b["x"]) and np.array_equal(a["qs"], b["qs"])
    for ca, cb in zip(a["calls"], b["calls"]):
        assert ca["kind"] == cb["kind"] and (ca.get("ids") is None or np.array_equal(ca["ids"], cb["ids"]))
    a, b = si.draw_mutation("ivf", 0, oracle), si.draw_mutation("ivf", 0, oracle)
    assert a["label"] == b["label"] and a["final_bytes"] == b["final_bytes"]


def test_exact_regimes(oracle):
    names = ("eligible d, N >= 8192", "eligible d, N < 8192, exact_filter = 1", "ineligible d", "N < k", "N not a multiple of 32",
             "N > the sample", "Q > a pass", "k > 32", "k-th and (k+1)-th similarity bit-equal", "refine_all")
    r = {n: [] for n in names}
    t = si.exj_min_targets()
    for kind in ("search_subset", "join"):
        r[f"{kind}: fewer known rows than EXJ_MIN_TARGETS"] = []
        r[f"{kind}: EXJ_MIN_TARGETS known rows or more"] = []
    n_kinds = len(si.EXACT_KINDS)
    after = np.zeros((n_kinds, n_kinds), int)      # after[a][b]: kind b directly after kind a
    for seed in si.SEEDS["exact"]:
        d = si.draw_exact(seed, oracle)
        assert d["label"].startswith(f"exact seed={seed} ") and 6 <= len(d["calls"]) <= 8, d["label"]
        assert d["d"] in si.EXACT_D and d["N"] in si.EXACT_N and d["Q"] in si.EXACT_Q and d["k"] in si.EXACT_K and d["exact_filter"] in (-1, 1)
        assert d["N"] * d["d"] * d["Q"] <= si.ORACLE_BUDGET or d["Q"] == min(si.EXACT_Q), d["label"]
        assert (np.diff(d["ids"]) > 0).all()
        dup = d["N"] - np.unique(d["x"], axis=0).shape[0]
        assert dup >= 1, (d["label"], "no duplicated row")
        el = si.filter_eligible(d["d"])
        facts = (el and d["N"] >= si.EXF_AUTO_ROWS, el and d["N"] < si.EXF_AUTO_ROWS and d["exact_filter"] == 1, not el, d["N"] < d["k"],
                 d["N"] % 32 != 0, d["N"] > si.exf_sample(), d["Q"] > si.exf_pass(), d["k"] > 32, bool(si.exact_ties(d, oracle)), d["refine_all"])
        for n, f in zip(names, facts):
            if f:
                r[n].append(seed)
        ks = [si.EXACT_KINDS.index(k) for k in d["kinds"]]
        for a, b in zip(ks, ks[1:]):
            assert a != b
            after[a, b] += 1
        for c in d["calls"]:
            if c["kind"] in ("search_subset", "join", "assign"):
                known = np.isin(c["ids"], d["ids"])
                assert (~known).any() and np.unique(c["ids"]).size < c["ids"].size, (d["label"], "a subset without unknown or repeated ids")
            if c["kind"] in ("search_subset", "join"):
                n = np.intersect1d(c["ids"], d["ids"]).size
                name = f"{c['kind']}: " + ("fewer known rows than EXJ_MIN_TARGETS" if n < t else "EXJ_MIN_TARGETS known rows or more")
                if seed not in r[name]:
                    r[name].append(seed)
    _table("exact", r)
    _none_empty(r)
    assert len(r["k-th and (k+1)-th similarity bit-equal"]) >= 2, r
    missing = [(si.EXACT_KINDS[a], si.EXACT_KINDS[b]) for a in range(n_kinds) for b in range(n_kinds) if a != b and not after[a, b]]
    assert not missing, f"never directly after one another: {missing}\nrows: the earlier call, columns: the later, order {si.EXACT_KINDS}\n{after}"


def test_rerank_regimes(oracle):
    r = {f"k*pvf = {k}*{p}": [] for k, p in si.PV_POOL}
    r.update({f"n_cand = {n}": [] for n in si.NCAND_POOL})
    r.update({n: [] for n in ("a candidate list with ids without a vector row", "a triple that is not searched", "a list with fillers",
                              "a triple with v3 - v1 + v2 = 0", "ivf", "pq", "pq subset", "a target without a query (assign)")})
    for seed in si.SEEDS["rerank"]:
        d = si.draw_rerank(seed, oracle)
        r[f"k*pvf = {d['k']}*{d['pvf']}"].append(seed)
        r[f"n_cand = {d['n_cand']}"].append(seed)
        r[d["kind"]].append(seed)
        pvs = [d["pv"]] + ([d["pv2"]] if d["kind"] == "pq" else [])
        if any((p["scored"] < p["candidates"]).any() for p in pvs):
            r["a candidate list with ids without a vector row"].append(seed)
        if any((p["lists"] < 0).any() for p in pvs) or (d["analogy"]["lists"] < 0).any():
            r["a list with fillers"].append(seed)
        if not d["analogy"]["valid"].all():
            r["a triple that is not searched"].append(seed)
            assert d["analogy"]["stats"]["searched"] == int(d["analogy"]["valid"].sum()) < d["triples"].shape[0]
        if d["triples"].shape[0] >= 3:
            ids, x = d["vec_pin"]
            v1, v2, v3 = (x[np.searchsorted(ids, i)] for i in d["triples"][2])
            assert not ((v3 - v1) + v2).any(), d["label"]
            r["a triple with v3 - v1 + v2 = 0"].append(seed)
        if d["kind"] == "pq":
            r["pq subset"].append(seed)
            if (d["assign_exp"][0] < 0).any():
                r["a target without a query (assign)"].append(seed)
    _table("rerank", r)
    _none_empty(r)


def test_shapes_bigk_and_join_regimes(oracle):
    r = {f"shape {s}": [] for s in si.SHAPES}
    for seed in si.SEEDS["shapes"]:
        d = si.draw_shapes(seed, oracle)
        assert d["N"] <= si.N_CAP and d["Q"] <= si.Q_CAP
        r[f"shape {d['shape']}"].append(seed)
    b = {n: [] for n in ("ivfadc: 512 < k <= 4096, equal distances across the k-th place", "pq: 512 < k <= 4096, equal distances across the k-th place",
                         "a join with 1024 < k*pvf <= 8192", "pq_search_in with fewer targets than k")}
    for seed in si.SEEDS["bigk"]:
        d = si.draw_bigk(seed, oracle)
        assert d["N"] <= si.N_CAP
        ot = oracle.ivf_table(*d["ivf_pin"])
        for c in d["ivf_calls"]:
            assert 512 < c["k"] <= 4096
            more = oracle.ivfadc_search_many(ot, d["qs"], c["k"] + 1, c["W"], sentinel=c["sentinel"], found_rule=c["rule"], n_threads=8)
            tied = (more["id"][:, c["k"]] >= 0) & (more["dist"][:, c["k"] - 1] == more["dist"][:, c["k"]])
            if tied.any() and seed not in b["ivfadc: 512 < k <= 4096, equal distances across the k-th place"]:
                b["ivfadc: 512 < k <= 4096, equal distances across the k-th place"].append(seed)
        op = oracle.pq_table(*d["pq_pin"])
        more = np.stack([oracle.pq_search(op, q, d["pq_k"] + 1) for q in d["qs"]])
        if ((more["id"][:, d["pq_k"]] >= 0) & (more["dist"][:, d["pq_k"] - 1] == more["dist"][:, d["pq_k"]])).any():
            b["pq: 512 < k <= 4096, equal distances across the k-th place"].append(seed)
        if d["pq_targets"].size < d["pq_k"]:
            b["pq_search_in with fewer targets than k"].append(seed)
        if d["join"] and all(1024 < c["k"] * c["pvf"] <= 8192 for c in d["join"]["calls"]):
            b["a join with 1024 < k*pvf <= 8192"].append(seed)
    j = {n: [] for n in ("duplicate multi-index centroids", "method 0", "method 1", "method 2", "target lists off", "more than one iteration")}
    for seed in si.SEEDS["join"]:
        d = si.draw_join(seed, oracle)
        assert d["N"] <= si.N_CAP and d["Q"] <= si.Q_CAP
        facts = {"duplicate multi-index centroids": seed % 4 == 1, "target lists off": any(not c["tl"] for c in d["calls"]),
                 "more than one iteration": any(c["iterations"] > 1 for c in d["calls"])}
        facts.update({f"method {m}": any(c["method"] == m for c in d["calls"]) for m in (0, 1, 2)})
        for n, f in facts.items():
            if f:
                j[n].append(seed)
    for title, regimes in (("shapes", r), ("bigk", b), ("join", j)):
        _table(title, regimes)
        _none_empty(regimes)


@pytest.mark.parametrize("kind", si.MUTATION_KINDS)
def test_mutation_regimes_and_refusals(oracle, kind):
    """Per kind: every operation, every ordered pair of distinct operations consecutively, an R or U that names an id an earlier
    step removed, (ivf) a U that changes a row's cell, and in every walk a step that changes the oracle's lists.  Every walk also
    runs through update_model alone: the refused step raises Refused and leaves the tables byte-identical, the applied steps
    return what the draw recorded and end in the draw's final state."""
    ops = "ARU" if kind == "vec" else "ARUC"
    r = {f"op {o}": [] for o in ops}
    r.update({f"{a} then {b}": [] for a in ops for b in ops if a != b})
    r.update({"an R or U names an id removed earlier": [], "a refused step": []})
    r.update({f"refused: {n}": [] for n in si.REFUSALS[kind]})
    if kind == "ivf":
        r["a U changes a row's cell"] = []
    for seed in si.SEEDS["mutation"]:
        d = si.draw_mutation(kind, seed, oracle)
        steps = d["steps"]
        assert len(steps) == si.MUTATION_STEPS and 3000 <= d["n0"] <= 5000, d["label"]
        assert sum(s["op"] == "refused" for s in steps) == 1 and sum(s["full"] for s in steps) == 4 and steps[-1]["full"] != (steps[-1]["op"] == "refused"), d["label"]
        assert any(s["bites"] for s in steps if s["op"] in "ARUC"), (d["label"], "no step changes the oracle's lists: the case does not bite")
        applied = [s["op"] for s in steps if s["op"] != "refused"]
        for o in applied:
            if seed not in r[f"op {o}"]:
                r[f"op {o}"].append(seed)
        for a, b in zip(applied, applied[1:]):
            if a != b and seed not in r[f"{a} then {b}"]:
                r[f"{a} then {b}"].append(seed)
        if any(s.get("names_removed", 0) for s in steps):
            r["an R or U names an id removed earlier"].append(seed)
        if kind == "ivf" and any(s.get("cells_changed", 0) for s in steps):
            r["a U changes a row's cell"].append(seed)
        model = si.mutation_model(kind, d["start"])
        for s in steps:
            assert s["size"] in si.MUTATION_SIZES or s["op"] in ("C", "refused"), d["label"]
            if s["op"] == "refused":
                was = si.model_bytes(kind, model)
                with pytest.raises(um.Refused):
                    si.apply_to_model(kind, model, s)
                assert si.model_bytes(kind, model) == was, (d["label"], "the refused step changed the model")
                r["a refused step"].append(seed)
                r[f"refused: {s['reason']}"].append(seed)
            else:
                assert si.apply_to_model(kind, model, s) == s["returns"], d["label"]
                if s["op"] == "A":
                    assert (np.diff(s["ids"]) > 0).all()
            assert model.N == s["N"], d["label"]
        assert si.model_bytes(kind, model) == d["final_bytes"], d["label"]
    _table(f"mutation {kind}", r)
    _none_empty(r)
