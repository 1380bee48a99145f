"""-m gpu: freddy_gpu_tokenize (include/freddy_gpu.h; csrc/tokenize.h) against the numpy model (tests/tokenize_model.py), bit for bit:
every case of tests/tokenize_inputs.py (three shapes; texts of 0 .. 4096 ids, unsorted, with duplicates, with unknown ids), both id
rules, with and without the normalisation, the counts too, and both forms of the normalisation kernel (option tokenize_unit).  Then
the limit of 4096 ids per text, an empty call, grids smaller than their work (grid_cus = 1 with 1 and 1 500 texts), a handle after
append_rows / remove_rows / update_rows against a fresh pin of the same rows, and a poisoned handle."""
import ctypes as C

import numpy as np
import pytest

import tokenize_inputs as ti
import tokenize_model as tm

pytestmark = pytest.mark.gpu
U = np.uint32
E_LIMIT, E_HIP = -5, -2


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def tables(gpu):
    out = {}
    for d in ti.SHAPES:
        ids, v = ti.table(d)
        out[d] = {"ids": ids, "v": v, "texts": ti.texts(ids), "vec": gpu.VectorIndex(ids, v)}
    yield out
    for t in out.values():
        t["vec"].close()


def _same(got, exp, what):
    gv, gc = got
    ev, ec = exp
    assert gv.shape == ev.shape and gv.dtype == np.float32, what
    assert np.array_equal(gc, ec), (what, "counts", np.flatnonzero(gc != ec)[:5].tolist())
    bad = np.flatnonzero((gv.view(U) != ev.view(U)).any(axis=1))
    assert bad.size == 0, (what, "texts whose vectors differ", bad[:8].tolist())


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("rule", [tm.TABLE_ORDER, tm.POSITIONAL])
@pytest.mark.parametrize("d", ti.SHAPES)
def test_every_case_equals_the_model(tables, oracle, d, rule, normalize):
    t = tables[d]
    vec, texts = t["vec"], [x for _, x in t["texts"]]
    exp = tm.tokenize(oracle, t["ids"], t["v"], texts, rule, normalize)
    assert not np.isnan(exp[0]).any()   # (no text of the list has a zero centroid)
    assert set(exp[1].tolist()) >= {0, 1, 2} and exp[1].max() > 1024 and (rule == tm.TABLE_ORDER or exp[1].max() == 4096)
    what = f"d={d} rule={rule} normalize={normalize}"
    got, names = _profiled(vec, lambda: vec.tokenize(texts, normalize=normalize, rule=rule))
    _same(got, exp, what)
    assert names == {"tok_resolve", "tok_rows", "tok_centroid"} | ({"tok_unit"} if normalize else set()), (what, sorted(names))
    # the (ids, offsets) form of the binding, and one text per call
    _same(vec.tokenize(ti.ragged(texts), normalize=normalize, rule=rule), exp, what + " ragged pair")
    for i in (0, 1, len(texts) - 4):
        _same(vec.tokenize([texts[i]], normalize=normalize, rule=rule), (exp[0][i:i + 1], exp[1][i:i + 1]), f"{what} text {i} alone")
    if normalize:   # both forms of the normalisation kernel (auto takes the wave form at this many texts)
        try:
            for unit in (1, 2):
                vec.set_option("tokenize_unit", unit)
                _same(vec.tokenize(texts, normalize=True, rule=rule), exp, f"{what} tokenize_unit={unit}")
        finally:
            vec.set_option("tokenize_unit", 0)


def test_a_text_of_4097_ids_is_refused_and_nothing_is_written(gpu, tables):
    t = tables[64]
    vec, lib = t["vec"], gpu.load()
    ids = np.resize(t["ids"], 3 + 4097 + 2).astype(np.int32)
    off = np.array([0, 3, 3 + 4097, 3 + 4097 + 2], np.int64)
    out, cnt = np.full((3, 64), 7.0, np.float32), np.full(3, 7, np.int32)
    (rc, names) = _profiled(vec, lambda: lib.freddy_gpu_tokenize(vec.h, gpu._p(ids), gpu._p(off), 3, 0, 1, gpu._p(out), gpu._p(cnt)))
    msg = lib.freddy_gpu_last_error().decode()
    assert rc == E_LIMIT and "text 1" in msg and "4097" in msg, (rc, msg)
    assert names == set() and np.all(out == 7.0) and np.all(cnt == 7)
    oi, ov = np.full((3, 2), 7, np.int32), np.full((3, 2), 7.0, np.float32)
    rc = lib.freddy_gpu_exact_search_texts(vec.h, gpu._p(ids), gpu._p(off), 3, 0, 1, 2, None, 0, gpu._p(cnt), gpu._p(oi), gpu._p(ov))
    assert rc == E_LIMIT and np.all(oi == 7) and np.all(ov == 7.0) and np.all(cnt == 7)
    # 4096 is served
    off[2] = 3 + 4096
    assert lib.freddy_gpu_tokenize(vec.h, gpu._p(ids), gpu._p(off), 2, 0, 1, gpu._p(out), gpu._p(cnt)) == 0 and cnt[1] > 0


def test_an_empty_call_launches_nothing(tables):
    vec = tables[300]["vec"]
    (v, c), names = _profiled(vec, lambda: vec.tokenize([]))
    assert v.shape == (0, 300) and c.shape == (0,) and names == set()


@pytest.mark.parametrize("d", [300, 25])
def test_grids_smaller_than_their_work(tables, oracle, d):
    """grid_cus = 1: eight workgroups at most -- 1 500 texts are 1 500 waves of tok_rows, 375 workgroups of tok_centroid and 24 of
    tok_unit, about 6 600 ids are 26 workgroups of tok_resolve: every grid loop goes round; and one text alone."""
    t = tables[d]
    vec, ids = t["vec"], t["ids"]
    rng = np.random.default_rng(77)
    texts = []
    for i in range(1500):
        L = int(rng.integers(0, 10))
        x = rng.choice(ids, size=L).astype(np.int32)
        if i % 7 == 3 and L:
            x[rng.integers(0, L)] = ids[-1] + 5 + i      # an unknown id
        if i % 31 == 5:
            x[:] = -3                                    # only unknown ids
        texts.append(x)
    assert sum(len(x) for x in texts) > 8 * 256 * 2
    for rule in (tm.TABLE_ORDER, tm.POSITIONAL):
        exp = tm.tokenize(oracle, ids, t["v"], texts, rule, True)
        assert (exp[1] == 0).sum() > 100
        base = vec.tokenize(texts, rule=rule)
        vec.set_option("grid_cus", 1)
        try:
            _same(vec.tokenize(texts, rule=rule), exp, f"d={d} rule={rule} 1500 texts grid_cus=1")
            _same(vec.tokenize(texts[8:9], rule=rule), (exp[0][8:9], exp[1][8:9]), f"d={d} rule={rule} one text grid_cus=1")
            for unit in (1, 2):
                vec.set_option("tokenize_unit", unit)
                _same(vec.tokenize(texts, rule=rule), exp, f"d={d} rule={rule} 1500 texts grid_cus=1 tokenize_unit={unit}")
        finally:
            vec.set_option("tokenize_unit", 0)
            vec.set_option("grid_cus", 0)
        _same(base, exp, f"d={d} rule={rule} 1500 texts")


def test_both_sides_of_the_threshold_between_the_normalisation_kernels(tables, oracle):
    """16 383 texts take the wave form of tok_unit, 16 384 the lane form (csrc/tokenize.h TOK_UNIT_LANES): the model's bits on both
    sides, at the default option.  One or two ids per text at d = 25."""
    t = tables[25]
    vec, ids = t["vec"], t["ids"]
    rng = np.random.default_rng(16384)
    pool = np.delete(ids, 5)   # (row 5 is all -0.0: alone it would be a zero centroid)
    texts = [rng.choice(pool, size=1 + (i & 1)).astype(np.int32) for i in range(16384)]
    texts[7] = np.empty(0, np.int32)
    texts[16383] = ids[3:5].copy()
    exp = tm.tokenize(oracle, ids, t["v"], texts, tm.POSITIONAL, True)
    _same(vec.tokenize(texts, rule=tm.POSITIONAL), exp, "16384 texts")
    _same(vec.tokenize(texts[:16383], rule=tm.POSITIONAL), (exp[0][:16383], exp[1][:16383]), "16383 texts")


def test_a_mutated_handle_equals_a_fresh_pin(gpu, tables, oracle):
    """append_rows, remove_rows (gaps the serial-id probe misses) and update_rows on the vector handle, then the same texts: the
    results of a fresh pin of the rows that are left, and the model's."""
    t = tables[64]
    ids, v = t["ids"], t["v"]
    texts = [x for _, x in t["texts"] if len(x) <= 257]
    h = gpu.VectorIndex(ids[:1500], v[:1500])
    try:
        h.append_rows(ids[1500:], vectors=v[1500:])
        gone = np.concatenate([ids[3:900:7], ids[1600::11]])
        assert h.remove_rows(gone) == gone.size
        keep = ~np.isin(ids, gone)
        ids2, v2 = ids[keep], v[keep].copy()
        changed = ids2[5::13]
        newv = (-v2[5::13][::-1]).copy()
        assert h.update_rows(changed, vectors=newv) == changed.size
        v2[5::13] = newv
        fresh = gpu.VectorIndex(ids2, v2)
        try:
            for rule in (tm.TABLE_ORDER, tm.POSITIONAL):
                exp = tm.tokenize(oracle, ids2, v2, texts, rule, True)
                assert 0 < (exp[1] == 0).sum() < len(texts)
                _same(h.tokenize(texts, rule=rule), exp, f"mutated handle rule={rule}")
                _same(fresh.tokenize(texts, rule=rule), exp, f"fresh pin rule={rule}")
        finally:
            fresh.close()
    finally:
        h.close()


def test_a_poisoned_handle_is_refused(gpu, tables):
    """A vector handle that a failed update_rows has poisoned (one of its allocations fails after the first write; tried from the
    last allocation down): FREDDY_E_HIP with the unpin message from all four entry points' vector handle, nothing launched, outputs
    untouched."""
    t = tables[64]
    ids, v, lib, P = t["ids"], t["v"], gpu.load(), gpu._p
    mutate = lambda h: h.update_rows(ids[:40], vectors=v[40:80])   # noqa: E731
    ref = gpu.VectorIndex(ids, v)
    c0 = gpu.alloc_stats().calls
    mutate(ref)
    A = gpu.alloc_stats().calls - c0
    ref.close()
    one_q, o1, o2 = v[:1], np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)
    bad = None
    for n in range(A, 0, -1):
        h = gpu.VectorIndex(ids, v)
        gpu.alloc_fail_nth(n)
        try:
            mutate(h)
        except gpu.FreddyGpuError as e:
            assert e.code == gpu.E_NOMEM, e
        finally:
            gpu.alloc_fail_nth(0)
        if lib.freddy_gpu_exact_search(h.h, P(one_q), 1, 0, None, 0, P(o1), P(o2)) == E_HIP:
            bad = h
            break
        h.close()
    assert bad is not None, f"none of the {A} allocations of update_rows, failed, poisons the handle"
    try:
        tok, off = ti.ragged([ids[:3], ids[5:6]])
        out, cnt = np.full((2, 64), 7.0, np.float32), np.full(2, 7, np.int32)
        oi, ov = np.full((2, 2), 7, np.int32), np.full((2, 2), 7.0, np.float32)
        bad.profile_enable(True)
        c0 = gpu.alloc_stats().calls
        assert lib.freddy_gpu_tokenize(bad.h, P(tok), P(off), 2, 0, 1, P(out), P(cnt)) == E_HIP
        assert "unpin it and pin again" in lib.freddy_gpu_last_error().decode()
        assert lib.freddy_gpu_exact_search_texts(bad.h, P(tok), P(off), 2, 0, 1, 2, None, 0, P(cnt), P(oi), P(ov)) == E_HIP
        assert "unpin it and pin again" in lib.freddy_gpu_last_error().decode()
        assert gpu.alloc_stats().calls == c0 and bad.profile_read() == {}
        assert np.all(out == 7.0) and np.all(cnt == 7) and np.all(oi == 7) and np.all(ov == 7.0)
    finally:
        bad.close()
