"""-m gpu: the searches over text vectors (freddy_gpu_ivfadc_search_texts, freddy_gpu_pq_search_texts, freddy_gpu_exact_search_texts;
the bindings search_texts).  The handles are those of tests/test_gpu_query_ids.py (the 300-d shape: ivf, pq and the vector table of
4999 rows with the ids 3 r + 1).  200 texts, empty ones and ones of unknown ids only among them; option tokenize_pass makes the
texts with a row list take two and a half passes.  Every list equals, bit for bit, the list of the public float entry point over the
vector freddy_gpu_tokenize returns for its text (which tests/test_gpu_tokenize.py compares with the model); the fillers sit exactly
where out_count == 0; with and without subset_ids, at k = 1, 5 and 600; and a permutation of a text's ids changes nothing under
FREDDY_QIDS_TABLE_ORDER."""
import numpy as np
import pytest

import query_ids_inputs as qi

pytestmark = pytest.mark.gpu
U = np.uint32
TO, POS = 0, 1
N_TEXTS = 200


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def handles(gpu):
    c = qi.case("d300_k256")
    h = {"c": c, "ivf": gpu.IVFIndex(*qi.ivf_args(c["ivf"])), "vec": gpu.VectorIndex(c["vec_ids"], c["vec_x"]),
         "pq": gpu.PQIndex(c["pq"]["codebook"], c["pq"]["ids"], c["pq"]["codes"])}
    yield h
    for n in ("ivf", "vec", "pq"):
        h[n].close()


def make_texts(vids, seed=3):
    """200 texts of 0 .. 12 ids of the table in any order, duplicates and unknown ids (3 r + 2 has no row) mixed in; every ninth is
    empty, every eleventh holds unknown ids only"""
    rng = np.random.default_rng(seed)
    texts = []
    for i in range(N_TEXTS):
        L = int(rng.integers(1, 13))
        x = rng.choice(vids, size=L).astype(np.int32)
        if i % 4 == 1 and L > 1:
            x[-1] = x[0]
        if i % 5 == 2:
            x[rng.integers(0, L)] += 1
        if i % 9 == 0:
            x = np.empty(0, np.int32)
        elif i % 11 == 0:
            x = (x // 3 * 3 + 2).astype(np.int32)
        texts.append(x)
    return texts


def _check(got, vecs_of, counts, search, filler, k, what):
    """got = (counts, ids, values) of a search_texts call; search(vectors) the float entry point"""
    gc, gi, gv = got
    assert np.array_equal(gc, counts), what
    live = counts > 0
    assert 0 < live.sum() < live.size
    ei, ev = search(np.ascontiguousarray(vecs_of[live]))
    assert gi.shape == (counts.size, k) and np.array_equal(gi[live], ei), (what, "ids differ from the float entry point's")
    assert np.array_equal(gv[live].view(U), ev.view(U)), (what, "value bits differ from the float entry point's")
    assert (gi[~live] == -1).all(), (what, "fillers")
    fv = gv[~live]
    assert (np.isneginf(fv).all() if np.isneginf(filler) else (fv == np.float32(filler)).all()), (what, "fillers")


def _with_passes(vec, n_live, call):
    """call() with tokenize_pass set so that the live texts take two and a half passes, then at the default"""
    p = int(n_live / 2.5)
    assert 2 * p < n_live < 3 * p
    vec.set_option("tokenize_pass", p)
    try:
        a = call()
    finally:
        vec.set_option("tokenize_pass", 0)
    return a, call()


def _equal(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(U), b[2].view(U)), what


@pytest.mark.parametrize("k", [1, 5, 600])
@pytest.mark.parametrize("rule", [TO, POS])
def test_ivfadc_search_texts(handles, k, rule):
    ivf, vec, c = handles["ivf"], handles["vec"], handles["c"]
    texts = make_texts(c["vec_ids"])
    vecs_of, counts = vec.tokenize(texts, rule=rule)
    W = c["W"]
    passes, whole = _with_passes(vec, int((counts > 0).sum()), lambda: ivf.search_texts(vec, texts, k, W, rule=rule))
    what = f"ivfadc k={k} rule={rule}"
    _check(passes, vecs_of, counts, lambda q: ivf.search(q, k, W), 1000.0, k, what + " in passes")
    _equal(passes, whole, what + ": one pass")
    if k == 5:   # another sentinel and found rule
        got = ivf.search_texts(vec, texts, k, W, sentinel=100.0, found_rule=1, rule=rule)
        _check(got, vecs_of, counts, lambda q: ivf.search(q, k, W, sentinel=100.0, found_rule=1), 100.0, k, what + " found_rule=1")


@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("k", [1, 5, 600])
def test_pq_search_texts(handles, k, subset):
    pq, vec, c = handles["pq"], handles["vec"], handles["c"]
    texts = make_texts(c["vec_ids"])
    sub = np.random.default_rng(8).choice(c["pq"]["ids"], size=1500, replace=False).astype(np.int32) if subset else None
    for rule in (TO, POS):
        vecs_of, counts = vec.tokenize(texts, rule=rule)
        passes, whole = _with_passes(vec, int((counts > 0).sum()), lambda: pq.search_texts(vec, texts, k, subset_ids=sub, rule=rule))
        what = f"pq k={k} subset={subset} rule={rule}"
        _check(passes, vecs_of, counts, lambda q: pq.search(q, k, subset_ids=sub), 100.0, k, what + " in passes")
        _equal(passes, whole, what + ": one pass")


@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("k", [1, 5, 600])
def test_exact_search_texts(handles, k, subset):
    vec, c = handles["vec"], handles["c"]
    texts = make_texts(c["vec_ids"])
    sub = np.random.default_rng(9).choice(c["vec_ids"], size=1500, replace=False).astype(np.int32) if subset else None
    for rule, normalize in ((TO, True), (POS, True), (TO, False)):
        vecs_of, counts = vec.tokenize(texts, normalize=normalize, rule=rule)
        passes, whole = _with_passes(vec, int((counts > 0).sum()),
                                     lambda: vec.search_texts(texts, k, normalize=normalize, subset_ids=sub, rule=rule))
        what = f"exact k={k} subset={subset} rule={rule} normalize={normalize}"
        _check(passes, vecs_of, counts, lambda q: vec.search(q, k, subset_ids=sub), -np.inf, k, what + " in passes")
        _equal(passes, whole, what + ": one pass")


def test_a_permutation_of_a_texts_ids_changes_nothing_in_table_order(handles):
    ivf, pq, vec, c = handles["ivf"], handles["pq"], handles["vec"], handles["c"]
    texts = make_texts(c["vec_ids"])
    rng = np.random.default_rng(21)
    shuffled = [rng.permutation(x).astype(np.int32) for x in texts]
    assert sum(not np.array_equal(a, b) for a, b in zip(texts, shuffled)) > 100
    va, ca = vec.tokenize(texts)
    vb, cb = vec.tokenize(shuffled)
    assert np.array_equal(ca, cb) and np.array_equal(va.view(U), vb.view(U))
    for name, call in (("ivfadc", lambda t: ivf.search_texts(vec, t, 5, c["W"])), ("pq", lambda t: pq.search_texts(vec, t, 5)),
                       ("exact", lambda t: vec.search_texts(t, 5))):
        _equal(call(texts), call(shuffled), name)
    # and it does change the vector of some text under POSITIONAL: the rule is not ignored
    pa, _ = vec.tokenize(texts, rule=POS)
    pb, _ = vec.tokenize(shuffled, rule=POS)
    assert not np.array_equal(pa.view(U), pb.view(U))


def test_texts_without_a_row_launch_no_search(handles):
    ivf, vec, c = handles["ivf"], handles["vec"], handles["c"]
    texts = [np.empty(0, np.int32), (c["vec_ids"][:5] + 1).astype(np.int32), np.array([-4, 2 ** 31 - 1], np.int32)]
    for h in (ivf, vec):
        h.profile_enable(True)
    try:
        cnt, gi, gd = ivf.search_texts(vec, texts, 4, c["W"], sentinel=77.0)
        assert set(ivf.profile_read()) == set() and set(vec.profile_read()) == {"tok_resolve", "tok_rows"}
    finally:
        for h in (ivf, vec):
            h.profile_enable(False)
    assert (cnt == 0).all() and (gi == -1).all() and (gd == np.float32(77.0)).all()
    cnt, gi, gs = vec.search_texts(texts, 4)
    assert (cnt == 0).all() and (gi == -1).all() and np.isneginf(gs).all()
