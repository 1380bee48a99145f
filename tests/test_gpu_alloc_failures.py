"""-m gpu: every allocation of every pin and every mutation fails once (the allocation seam, csrc/alloc_hook.h), and the handle is
looked at afterwards.

A scenario is one call on one table shape.  It runs once with the seam's counter read around it: A = the allocations the call
makes, which must reach the FLOOR read off the code (written beside every scenario with its derivation -- a seam that is not
wired in cannot pass with an empty sweep).  Then for EVERY n in 1 .. A a fresh handle is pinned, the n-th allocation from now is
made to fail, and the call is made.  What must hold (include/freddy_gpu.h, "the contract of a failed call"), checked in this
order so that no kernel runs on a handle the host-side checks already show to be inconsistent:
  1. the call returns FREDDY_E_NOMEM and freddy_gpu_last_error() says something; exactly one allocation failed;
  2. a failed pin leaves *out NULL and the live allocations (count, bytes, digest) as they were before it;
  3. a failed mutation leaves the handle INTACT or POISONED -- asked with a call that is refused before anything is launched in
     either state (k = 0: FREDDY_E_HIP "unpin it and pin again" from a poisoned handle, FREDDY_E_ARG from a healthy one):
       poisoned: every search entry point of the kind refuses with that message, allocating nothing; unpin works;
       intact:   index_bytes and the live allocations are those of before the call (plus the scratch a scenario lists by name);
  4. only then, on an intact handle: the searches answer as before the call, bit for bit (lists that were held to the oracle
     once per scenario); the same call made again succeeds; the handle then equals a fresh pin of the new table in ids, float
     bits, the kernels the profile names, index_bytes, and bound_violations() == 0 (that fresh pin was held to the oracle too);
  5. after unpin the live allocations are those of before the pin.
Scenarios that promise "intact" (everything is built beside the old arrays and swapped in last) fail if any n poisons.
The tables are the smallest the mutation tests use; the expected tables come from mutation_model / removal_model / update_model
/ statistics_model."""
import ctypes as C

import numpy as np
import pytest

import analogy_model as am
import statistics_model as sm
import update_model as um          # (the classes of mutation_model with remove() and update())
import util
from test_gpu_mutation import _exact_same, _ivf_source, _ivpq_source, _nudged, _pq_source, _vec_table

pytestmark = pytest.mark.gpu

UNPIN = "unpin it and pin again"


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def helpers(gpu):
    """Small vector handles for the calls that take two handles (search_pv, the approximate analogies), pinned BEFORE tracking
    starts so that they never show in a live count; then tracking on for the module."""
    vecs = {}
    for d in (300, 35, 100):
        x, ids = _vec_table(d, 64)
        vecs[d] = gpu.VectorIndex(ids, x)
    gpu.alloc_fail_nth(0)
    gpu.alloc_track(True)
    yield vecs
    gpu.alloc_fail_nth(0)
    gpu.alloc_track(False)
    for v in vecs.values():
        v.close()


def _live(gpu):
    st = gpu.alloc_stats()
    return st.live, st.live_bytes, st.digest


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).tobytes()


def _same_answers(got, ref, what):
    assert len(got) == len(ref), what
    for j, (g, r) in enumerate(zip(got, ref)):
        assert len(g) == len(r), (what, j)
        for u, (x, y) in enumerate(zip(g, r)):
            if isinstance(x, np.ndarray):
                assert x.shape == y.shape and _bits(x) == _bits(y), f"{what}: answer {j} part {u} differs"
            else:
                assert x == y, f"{what}: answer {j} part {u}: {x} != {y}"


# =======================================================================================
# the four kinds: how to pin a model, what to ask it, what the oracle says, who must refuse
# =======================================================================================
class Kind:
    def __init__(self, name, pin, answers, check_oracle, probe, refusing, same_bytes=True):
        self.name, self.pin, self.answers, self.check_oracle, self.probe, self.refusing, self.same_bytes = name, pin, answers, check_oracle, probe, refusing, same_bytes


def _profiled(idx, calls):
    idx.profile_enable(True)
    out = [c() for c in calls]
    names = sorted(idx.profile_read())
    idx.profile_enable(False)
    return out, names


# ---- pq ----
def _pq_inputs(model_ids, x, d):
    rng = np.random.default_rng(d)
    qs = np.ascontiguousarray(x[rng.choice(600, 20, replace=False)])
    sub = np.concatenate([model_ids[::7], model_ids[:25], [1, 3, -5, 10 ** 8 + 1]]).astype(np.int32)
    gv = np.ascontiguousarray(x[rng.choice(600, 5, replace=False)]); gv[3] = gv[0]
    return qs, sub, gv


def _pq_kind(gpu, helpers, x, d, all_ids):
    qs, sub, gv = _pq_inputs(all_ids, x, d)

    def answers(idx):
        return _profiled(idx, [lambda: idx.search(qs[:1], 5), lambda: idx.search(qs, 7), lambda: idx.search(qs, 5, sentinel=1000.0, subset_ids=sub),
                               lambda: idx.grouping(gv, None)])

    def check_oracle(oracle, model, ans, what):
        ot = model.oracle_table(oracle)
        util.assert_same_lists(ans[0][0], ans[0][1], oracle.pq_search(ot, qs[0], 5)[None], what + " one query")
        util.assert_same_lists(ans[1][0], ans[1][1], np.stack([oracle.pq_search(ot, q, 7) for q in qs]), what + " batch")
        util.assert_same_lists(ans[2][0], ans[2][1], oracle.pq_search_in_batch(ot, qs, 5, sub), what + " subset")
        ei, eg = oracle.grouping_pq(ot, gv, model.ids)
        assert np.array_equal(ans[3][0], ei) and np.array_equal(ans[3][1], eg), what + " grouping"

    def probe(idx):
        oi, od = np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)
        return idx.lib.freddy_gpu_pq_search(idx.h, gpu._p(qs), 1, 0, C.c_float(100.0), None, 0, gpu._p(oi), gpu._p(od))

    def refusing(idx):
        import torch
        dq = torch.from_numpy(qs).cuda()
        oi = torch.zeros((len(qs), 7), dtype=torch.int32, device="cuda"); od = torch.zeros((len(qs), 7), dtype=torch.float32, device="cuda")
        tr = np.array([[all_ids[0], all_ids[1], all_ids[2]]], np.int32)
        return [lambda: idx.search(qs[:1], 5), lambda: idx.search(qs, 7), lambda: idx.search(qs, 5, sentinel=1000.0, subset_ids=sub),
                lambda: idx.grouping(gv, None), lambda: idx.assign(qs, all_ids[:50]),
                lambda: idx.search_dev(dq.data_ptr(), len(qs), 7, 100.0, oi.data_ptr(), od.data_ptr()),
                lambda: idx.search_pv(helpers[d], qs, 3, 4), lambda: idx.analogy(helpers[d], tr, 2)]

    return Kind("pq", lambda m: gpu.PQIndex(*m.pin_args()), answers, check_oracle, probe, refusing)


# ---- ivf ----
def _ivf_kind(gpu, helpers, x, d, devices=None):
    rng = np.random.default_rng(d + 1)
    qs = np.ascontiguousarray(x[rng.choice(450, 24, replace=False)])

    def answers(idx):
        return _profiled(idx, [lambda: idx.search(qs, 5, 3), lambda: idx.search(qs[-1:], 5, 3), lambda: idx.search(qs, 30, 1)])

    def check_oracle(oracle, model, ans, what):
        ot = model.oracle_table(oracle)
        util.assert_same_lists(ans[0][0], ans[0][1], oracle.ivfadc_search_many(ot, qs, 5, 3), what + " batch")
        util.assert_same_lists(ans[1][0], ans[1][1], oracle.ivfadc_search_many(ot, qs[-1:], 5, 3), what + " one query")
        util.assert_same_lists(ans[2][0], ans[2][1], oracle.ivfadc_search_many(ot, qs, 30, 1), what + " k = 30, W = 1")

    def probe(idx):
        oi, od = np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)
        return idx.lib.freddy_gpu_ivfadc_search(idx.h, gpu._p(qs), 1, 0, 3, C.c_float(1000.0), 0, gpu._p(oi), gpu._p(od))

    def refusing(idx):
        import torch
        dq = torch.from_numpy(qs).cuda()
        oi = torch.zeros((len(qs), 5), dtype=torch.int32, device="cuda"); od = torch.zeros((len(qs), 5), dtype=torch.float32, device="cuda")
        st = torch.zeros(4, dtype=torch.int32, device="cuda")
        tr = np.array([[1, 2, 3]], np.int32)
        calls = [lambda: idx.search(qs, 5, 3), lambda: idx.search(qs[-1:], 5, 3),
                 lambda: idx.search_dev(dq.data_ptr(), len(qs), 5, 3, 1000.0, 0, oi.data_ptr(), od.data_ptr(), st.data_ptr())]
        if devices is None:   # (the two-handle calls take no handle with replicas: refused for that reason before this one)
            calls += [lambda: idx.search_pv(helpers[d], qs, 3, 4, 3), lambda: idx.analogy(helpers[d], tr, 2)]
        return calls

    return Kind("ivf", lambda m: gpu.IVFIndex(*m.pin_args(), devices=devices), answers, check_oracle, probe, refusing)


# ---- ivpq ----
def _ivpq_kind(gpu, x, with_vectors, all_ids):
    rng = np.random.default_rng(31)
    qs = np.ascontiguousarray(x[rng.choice(2500, 12, replace=False)])
    targets = np.concatenate([all_ids[rng.choice(3000, 500, replace=False)], all_ids[3000:3065], all_ids[:20], [10 ** 8, -4]]).astype(np.int32)
    methods = (0, 1, 2) if with_vectors else (0,)

    def answers(idx):
        return _profiled(idx, [lambda m=m: idx.knn_join(qs, 5, targets, 3, 20, m) for m in methods] + [lambda: idx.knn_join(qs, 10, targets, 1, 3, 0, use_target_lists=False, confidence=0.3)])

    def check_oracle(oracle, model, ans, what):
        ot = model.oracle_table(oracle)
        for m, a in zip(methods, ans):
            exp, it = oracle.ivpq_search_in(ot, qs, 5, targets, 3, 20, m)
            assert a[2] == it, (what, m, a[2], it)
            util.assert_same_lists(a[0], a[1], exp, f"{what} method {m}")
        exp, it = oracle.ivpq_search_in(ot, qs, 10, targets, 1, 3, 0, use_target_lists=False, confidence=0.3)
        assert ans[-1][2] == it, (what, ans[-1][2], it)
        util.assert_same_lists(ans[-1][0], ans[-1][1], exp, what + " no target lists")

    def probe(idx):
        oi, od, it = np.empty((1, 1), np.int32), np.empty((1, 1), np.float32), C.c_int32(0)
        return idx.lib.freddy_gpu_knn_join(idx.h, gpu._p(qs), 1, 0, gpu._p(targets), targets.size, 3, 20, 0, 1, C.c_float(0.8), 10000000,
                                           gpu._p(oi), gpu._p(od), C.byref(it))

    def refusing(idx):
        return [lambda m=m: idx.knn_join(qs, 5, targets, 3, 20, m) for m in methods] + \
               [lambda: idx.create_statistics(None, install=False), lambda: idx.create_statistics(targets, install=True), lambda: idx.statistics(),
                lambda: idx.set_statistics(np.ones(idx.cells + 1, np.float32))]

    return Kind("ivpq", lambda m: gpu.IVPQIndex(*m.pin_args()), answers, check_oracle, probe, refusing)


# ---- vectors ----
def _vec_kind(gpu, x, ids, d, n0):
    rng = np.random.default_rng(d + 2)
    qs = np.ascontiguousarray(x[rng.choice(n0, 10, replace=False)]); qs[1] = -qs[1]
    triples = ids[rng.integers(0, 500, size=(5, 3))].copy()
    triples[2, 0] = 4                                   # an id that is never known
    sub = np.concatenate([ids[rng.choice(n0, 150, replace=False)], ids[n0 - 70::3], ids[:10], [4, 10 ** 8]]).astype(np.int32)
    modes = (1, -1)                                      # the filter forced (where the shape has it) and the library's own choice

    def answers(idx):
        calls = []
        for mode in modes:
            calls.append(lambda mode=mode: idx.set_option("exact_filter", mode) or idx.search(qs, 5))
            calls.append(lambda: idx.search(qs, 5, subset_ids=sub))
            calls.append(lambda: idx.analogy(triples, k=4, method="3cosadd"))
        return _profiled(idx, calls)

    def check_oracle(oracle, model, ans, what):
        xv, iv = model.oracle_table(oracle)
        x_t = np.ascontiguousarray(xv.T)
        full = [oracle.exact_knn(xv, iv, q, 5) for q in qs]
        part = [oracle.exact_knn(xv, iv, q, 5, sub) for q in qs]
        ei, es = am.model(xv, iv, triples, 4, "3cosadd", x_t=x_t)
        for j, mode in enumerate(modes):
            a, b, c = ans[3 * j:3 * j + 3]
            _exact_same(a[0], a[1], full, 5, f"{what} exact_filter={mode}")
            _exact_same(b[0], b[1], part, 5, f"{what} exact_filter={mode} subset")
            assert np.array_equal(c[0], ei) and np.array_equal(c[1].view(np.uint64), es.view(np.uint64)), f"{what} exact_filter={mode} 3cosadd"

    def probe(idx):
        oi, od = np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)
        return idx.lib.freddy_gpu_exact_search(idx.h, gpu._p(qs), 1, 0, None, 0, gpu._p(oi), gpu._p(od))

    def refusing(idx):
        return [lambda: idx.search(qs, 5), lambda: idx.search(qs, 5, subset_ids=sub), lambda: idx.analogy(triples, k=4, method="3cosadd"),
                lambda: idx.analogy(triples, k=4, method="3cosmul"), lambda: idx.join(qs, 5, sub), lambda: idx.assign(qs, sub)]

    # (index_bytes of a vector handle counts the CAPACITY of the fragment-order copy, which is allocated with an eighth of headroom
    # and kept -- include/freddy_gpu.h on remove_rows; an append that fits the headroom leaves it, a fresh pin sizes it anew -- so the
    # figure is not a fresh pin's in either direction.  What is held instead: the figure after the call made again equals the figure
    # after the call made the first time; the other kinds equal a fresh pin's)
    return Kind("vec", lambda m: gpu.VectorIndex(*m.pin_args()), answers, check_oracle, probe, refusing, same_bytes=False)


# =======================================================================================
# the sweeps
# =======================================================================================
SUMMARY = []


def _report(name, A, floor, states):
    line = f"alloc-failure sweep {name}: A = {A} allocations (floor {floor}), states {''.join(states) or '-'}  [I = intact, P = poisoned, N = pin: NULL]"
    SUMMARY.append(line)
    print(line)


def _failing(gpu, n, call):
    """call() with the n-th allocation from now failing -> the error it raised (None: it succeeded); the seam is disarmed afterwards"""
    failed0 = gpu.alloc_stats().failed
    gpu.alloc_fail_nth(n)
    err = None
    try:
        call()
    except gpu.FreddyGpuError as e:
        err = e
    finally:
        gpu.alloc_fail_nth(0)
    return err, gpu.alloc_stats().failed - failed0


def _assert_nomem(gpu, err, failed, what):
    assert err is not None, f"{what}: the call succeeded although one of its allocations was to fail"
    assert failed == 1, f"{what}: {failed} allocations failed, one was armed"
    assert err.code == gpu.E_NOMEM, f"{what}: {err}"
    assert gpu.load().freddy_gpu_last_error().decode().strip(), f"{what}: no message"


def _sweep_pin(gpu, name, cls, args, kw, floor):
    s0 = _live(gpu)
    c0 = gpu.alloc_stats().calls
    idx = cls(*args, **kw)
    A = gpu.alloc_stats().calls - c0
    idx.close()
    assert _live(gpu) == s0, f"{name}: unpin left allocations behind"
    assert A >= floor, f"{name}: the pin made {A} allocations through the seam, the code allocates at least {floor}"
    for n in range(1, A + 1):
        obj = cls.__new__(cls)
        err, failed = _failing(gpu, n, lambda: obj.__init__(*args, **kw))
        _assert_nomem(gpu, err, failed, f"{name} n={n}")
        assert obj.h.value is None, f"{name} n={n}: *out is not NULL after a failed pin"
        assert _live(gpu) == s0, f"{name} n={n}: the failed pin left allocations behind: {_live(gpu)} vs {s0}"
    _report(name, A, floor, ["N"] * A)


def _sweep_mutation(gpu, oracle, name, kind, make_model, mutate, mutate_model, floor, intact, kept=()):
    """kept: (live count, live bytes) a failed call may legitimately leave beyond the snapshot -- scratch the scenario names"""
    s0 = _live(gpu)
    before_model = make_model()
    ref = kind.pin(before_model)
    before, _ = kind.answers(ref)
    kind.check_oracle(oracle, before_model, before, f"{name}: before the call")
    ref.close()
    # the call once, counted, on a cold handle as every sweep step makes it; then the new table against the oracle and a fresh pin
    done = kind.pin(before_model)
    c0 = gpu.alloc_stats().calls
    mutate(done)
    A = gpu.alloc_stats().calls - c0
    assert A >= floor, f"{name}: the call made {A} allocations through the seam, the code allocates at least {floor}"
    after_model = make_model(); mutate_model(after_model)
    after, after_names = kind.answers(done)
    kind.check_oracle(oracle, after_model, after, f"{name}: after the call")
    fresh = kind.pin(after_model)
    fresh_ans, fresh_names = kind.answers(fresh)
    _same_answers(after, fresh_ans, f"{name}: against a fresh pin")
    assert after_names == fresh_names, (name, after_names, fresh_names)
    assert done.nbytes == fresh.nbytes or not kind.same_bytes, (name, done.nbytes, fresh.nbytes)
    assert done.bound_violations() == 0 and fresh.bound_violations() == 0
    nbytes_after = done.nbytes
    done.close(); fresh.close()
    assert _live(gpu) == s0, f"{name}: unpin left allocations behind"
    states = []
    for n in range(1, A + 1):
        what = f"{name} n={n}/{A}"
        idx = kind.pin(before_model)
        nb0, live0 = idx.nbytes, _live(gpu)
        err, failed = _failing(gpu, n, lambda: mutate(idx))
        _assert_nomem(gpu, err, failed, what)
        rc = kind.probe(idx)                              # (refused before anything is launched, whatever the state)
        assert rc in (-1, -2), (what, rc)
        if rc == -2:                                      # poisoned
            assert UNPIN in gpu.load().freddy_gpu_last_error().decode(), what
            assert not intact, f"{what}: the call builds beside the old arrays and must leave the handle intact, it is poisoned"
            c1 = gpu.alloc_stats().calls
            for j, call in enumerate(kind.refusing(idx)):
                with pytest.raises(gpu.FreddyGpuError, match=UNPIN):
                    call()
            assert gpu.alloc_stats().calls == c1, f"{what}: a refused search allocated"
            states.append("P")
        else:                                             # intact: the host-side figures first, searches only then
            assert idx.nbytes == nb0, f"{what}: index_bytes moved from {nb0} to {idx.nbytes} in a call that failed"
            now = _live(gpu)
            extra = (now[0] - live0[0], now[1] - live0[1])
            assert extra == (0, 0) or extra in kept, f"{what}: live allocations moved by {extra} in a call that failed (allowed: {kept})"
            assert extra != (0, 0) or now[2] == live0[2], f"{what}: the live set changed (digest) in a call that failed"
            got, _ = kind.answers(idx)
            _same_answers(got, before, f"{what}: the searches after the failed call")
            mutate(idx)                                   # the same call, nothing armed
            got, names = kind.answers(idx)
            _same_answers(got, after, f"{what}: after the call made again")
            assert names == after_names, (what, names, after_names)
            assert idx.nbytes == nbytes_after, (what, idx.nbytes, nbytes_after)
            assert idx.bound_violations() == 0, what
            states.append("I")
        idx.close()
        assert _live(gpu) == s0, f"{what}: unpin left allocations behind: {_live(gpu)} vs {s0}"
    _report(name, A, floor, states)
    return states


# =======================================================================================
# scenarios.  FLOORS: device arrays the code path allocates, counted in postgres-word2vec_amd/csrc (pin.hip and mutate.h / mutate_host.h unless said otherwise)
# =======================================================================================
#   derive_codebook_tables_into: cbT always; pq / ivf of the filter shape (m = 12, S = 25): cbR, pmax, cmaxp, cbF (+ cbP: ivf, K <= 1024)
#   pack_lists: blk_cell, blk_off, list_off, packed, pos = 5;  make_packed8 (K <= 256, m = 12): 1;  make_row_terms (cbR): 1
#   append_packed_rows: packed, pos, blk_cell, blk_off, list_off (stage_plan) + the staged slot, row_pos, codes = 8
#   remove_packed_rows: d_rm, keep_mask, keep_cnt, prefix, list_keep, d_max = 6, then packed, pos, blk_cell, blk_off, list_off (stage_plan) = 5
#   locate_packed_rows: 3;  rewrite_packed_rows: 3
PQ_SHAPES = {"300x12x256": ((300, 12, 256), 4200), "35x7x16": ((35, 7, 16), 700)}
PQ_FLOORS = {   # (pin, append, remove, update_rows, update_codebook)
    "300x12x256": (5 + 1 + 5 + 1,      # codebook tables 5, ids, pack_lists 5, packed8
                   8 + 1 + 1,          # append_packed_rows 8, packed8, ids
                   2 + 11 + 1,         # d_rm + the gathered ids, remove_packed_rows 11, packed8
                   3 + 3 + 1,          # locate, rewrite, packed8
                   5),                 # cbT, cbR, pmax, cmaxp, cbF
    "35x7x16": (1 + 1 + 5, 8 + 1, 2 + 11, 3 + 3, 1),
}
IVF_SHAPES = {"300x12x256x32": ((300, 12, 256, 32), 600), "100x5x64x16": ((100, 5, 64, 16), 500)}
IVF_FLOORS = {   # pin_ivf: coarse, coarseT, coarseH, coarseP, cn2, viol = 6
    "300x12x256x32": (6 + 6 + 5 + 1 + 1,   # + cbT, cbP, cbR, pmax, cmaxp, cbF; pack_lists; packed8; rterm
                      8 + 1 + 1,           # append_packed_rows, packed8, rterm
                      11 + 1 + 1,          # remove_packed_rows, packed8, rterm
                      3 + 3,               # locate, rewrite (rows that stay in their cell) at least
                      6 + 1),              # the six codebook tables and the row terms that follow them
    "100x5x64x16": (6 + 2 + 5, 8, 11, 3 + 3, 2),   # cbT and cbP only; no packed8, no rterm
}
IVPQ_FLOORS = {  # join.hip join_pin: cbT, coarseT, ids, codes, cell, d_stats, markbits (+ vectors)
    True: (8, 5, 6, 4), False: (7, 4, 5, 3),    # (pin, append: the grown arrays + markbits, remove: d_rm + markbits + the gathered arrays, update_rows: d_rows + a staged copy per array)
}
VEC_SHAPES = {"d300": (300, 8300), "d35": (35, 700)}
VEC_FLOORS = {   # exact.hip pin_vectors: xb, ids, the staging slice, the row-major copy (+ exf_small and the fragment copy where d % 4 == 0)
    "d300": (4 + 2, 3, 4, 2), "d35": (4, 3, 4, 2),   # (pin, append: xb + rows + ids, remove: d_rm + ids + rows + xb, update_rows: d_rows + d_src)
}


def _pq_setup(gpu, helpers, shape):
    (d, m, K), n0 = PQ_SHAPES[shape]
    cb, ids, codes, x = _pq_source(d, m, K)
    kind = _pq_kind(gpu, helpers, x, d, ids[:n0 + 65])
    return kind, (lambda: um.PQModel(cb, ids[:n0], codes[:n0])), cb, ids, codes, n0


@pytest.mark.parametrize("shape", list(PQ_SHAPES))
def test_pin_pq(gpu, helpers, shape):
    kind, make, *_ = _pq_setup(gpu, helpers, shape)
    _sweep_pin(gpu, f"pin_pq {shape}", gpu.PQIndex, make().pin_args(), {}, PQ_FLOORS[shape][0])


@pytest.mark.parametrize("call", ["append_rows", "remove_rows", "update_rows", "update_codebook"])
@pytest.mark.parametrize("shape", list(PQ_SHAPES))
def test_pq_mutation(gpu, helpers, oracle, shape, call):
    kind, make, cb, ids, codes, n0 = _pq_setup(gpu, helpers, shape)
    rng = np.random.default_rng(n0)
    gone = np.concatenate([ids[rng.choice(n0, 70, replace=False)], [1, 10 ** 8]]).astype(np.int32)
    upd = ids[rng.choice(n0, 40, replace=False)]
    upd_codes = codes[rng.choice(n0, 40, replace=False)]
    cb2 = _nudged(cb, 7)
    mut = {"append_rows": (lambda i: i.append_rows(ids[n0:n0 + 65], codes=codes[n0:n0 + 65]), lambda m: m.append(ids[n0:n0 + 65], codes[n0:n0 + 65]), True),
           "remove_rows": (lambda i: i.remove_rows(gone), lambda m: m.remove(gone), True),
           "update_rows": (lambda i: i.update_rows(upd, codes=upd_codes), lambda m: m.update(upd, upd_codes), False),   # in place: poisoned after the first write
           "update_codebook": (lambda i: i.update_codebook(cb2), lambda m: m.update_codebook(cb2), True)}[call]
    floor = PQ_FLOORS[shape][1 + ["append_rows", "remove_rows", "update_rows", "update_codebook"].index(call)]
    states = _sweep_mutation(gpu, oracle, f"pq {shape} {call}", kind, make, mut[0], mut[1], floor, mut[2])
    if call == "update_rows":
        assert "I" in states and "P" in states, states   # the locate step fails before anything is written, the rewrite after


def _ivf_setup(gpu, helpers, shape, devices=None):
    (d, m, K, Cn), n0 = IVF_SHAPES[shape]
    coarse, cb, ids, cell, codes, x = _ivf_source(d, m, K, Cn)
    kind = _ivf_kind(gpu, helpers, x, d, devices)
    return kind, (lambda: um.IVFModel.from_rows(coarse, cb, ids[:n0], cell[:n0], codes[:n0])), cb, ids, cell, codes, n0, Cn


@pytest.mark.parametrize("shape", list(IVF_SHAPES))
def test_pin_ivf(gpu, helpers, shape):
    kind, make, *_ = _ivf_setup(gpu, helpers, shape)
    _sweep_pin(gpu, f"pin_ivf {shape}", gpu.IVFIndex, make().pin_args(), {}, IVF_FLOORS[shape][0])


def test_pin_ivf_multi_same_device_twice(gpu, helpers):
    """two complete pins behind one handle: a failure in the second one frees the first as well"""
    kind, make, *_ = _ivf_setup(gpu, helpers, "300x12x256x32")
    _sweep_pin(gpu, "pin_ivf_multi [0, 0]", gpu.IVFIndex, make().pin_args(), {"devices": [0, 0]}, 2 * IVF_FLOORS["300x12x256x32"][0])


@pytest.mark.parametrize("call", ["append_rows", "remove_rows", "update_rows", "update_codebook"])
@pytest.mark.parametrize("shape", list(IVF_SHAPES))
def test_ivf_mutation(gpu, helpers, oracle, shape, call):
    kind, make, cb, ids, cell, codes, n0, Cn = _ivf_setup(gpu, helpers, shape)
    rng = np.random.default_rng(n0 + 1)
    gone = np.concatenate([ids[rng.choice(n0, 70, replace=False)], [10 ** 8]]).astype(np.int32)
    rows = rng.choice(n0, 40, replace=False)
    upd, upd_codes = ids[rows], codes[rng.choice(n0, 40, replace=False)]
    upd_cell = cell[rows].copy(); upd_cell[::2] = (upd_cell[::2] + 1) % Cn      # half of the rows move to another cell
    cb2 = _nudged(cb, 8)
    sl = slice(n0, n0 + 65)
    mut = {"append_rows": (lambda i: i.append_rows(ids[sl], coarse_id=cell[sl], codes=codes[sl]), lambda m: m.append(ids[sl], cell[sl], codes[sl]), True),
           "remove_rows": (lambda i: i.remove_rows(gone), lambda m: m.remove(gone), True),
           "update_rows": (lambda i: i.update_rows(upd, coarse_id=upd_cell, codes=upd_codes), lambda m: m.update(upd, upd_cell, upd_codes), False),
           "update_codebook": (lambda i: i.update_codebook(cb2), lambda m: m.update_codebook(cb2), True)}[call]
    floor = IVF_FLOORS[shape][1 + ["append_rows", "remove_rows", "update_rows", "update_codebook"].index(call)]
    states = _sweep_mutation(gpu, oracle, f"ivf {shape} {call}", kind, make, mut[0], mut[1], floor, mut[2])
    if call == "update_rows":
        assert "I" in states and "P" in states, states


def test_ivf_two_replicas_append(gpu, helpers, oracle):
    """The same device twice behind one handle: a failure on the primary leaves the handle as it was (no device has changed), a
    failure on the replica comes after the primary has changed and poisons it."""
    kind, make, cb, ids, cell, codes, n0, Cn = _ivf_setup(gpu, helpers, "300x12x256x32", devices=[0, 0])
    sl = slice(n0, n0 + 65)
    one = IVF_FLOORS["300x12x256x32"][1]
    states = _sweep_mutation(gpu, oracle, "ivf two replicas append_rows", kind, make, lambda i: i.append_rows(ids[sl], coarse_id=cell[sl], codes=codes[sl]),
                             lambda m: m.append(ids[sl], cell[sl], codes[sl]), 2 * one, False)
    half = len(states) // 2
    assert states[:half] == ["I"] * half and states[half:] == ["P"] * (len(states) - half), states


def _ivpq_setup(gpu, with_vectors):
    t, x = _ivpq_source(True)
    n0 = 3000
    ids = np.arange(1, 8001, dtype=np.int32)
    vec = t["vectors"] if with_vectors else None
    kind = _ivpq_kind(gpu, x, with_vectors, ids)
    make = lambda: um.IVPQModel(t["codebook"], t["coarse"], ids[:n0], t["coarse_id"][:n0], t["codes"][:n0], None if vec is None else vec[:n0], t["stats"])
    return kind, make, t, ids, vec, n0


@pytest.mark.parametrize("with_vectors", [True, False], ids=["vectors", "codes-only"])
def test_pin_ivpq(gpu, helpers, with_vectors):
    kind, make, *_ = _ivpq_setup(gpu, with_vectors)
    _sweep_pin(gpu, f"pin_ivpq 300x30x32xkc8 vectors={with_vectors}", gpu.IVPQIndex, make().pin_args(), {}, IVPQ_FLOORS[with_vectors][0])


@pytest.mark.parametrize("call", ["append_rows", "remove_rows", "update_rows", "update_codebook", "set_statistics", "create_statistics"])
@pytest.mark.parametrize("with_vectors", [True, False], ids=["vectors", "codes-only"])
def test_ivpq_mutation(gpu, helpers, oracle, with_vectors, call):
    kind, make, t, ids, vec, n0 = _ivpq_setup(gpu, with_vectors)
    rng = np.random.default_rng(5)
    sl = slice(n0, n0 + 65)
    take = lambda a, s: None if a is None else a[s]
    gone = np.concatenate([ids[rng.choice(n0, 70, replace=False)], [10 ** 8]]).astype(np.int32)
    rows, src = rng.choice(n0, 40, replace=False), rng.choice(n0, 40, replace=False)
    cb2 = _nudged(t["codebook"], 9)
    cells = t["stats"].size - 1
    new_stats = t["stats"][::-1].copy(); new_stats[-1] = t["stats"][-1]
    col = np.concatenate([ids[rng.choice(n0, 900, replace=True)], [10 ** 8]]).astype(np.int32)   # a column of tokens: ids with their multiplicity

    def model_create(m):
        m.stats = sm.create_statistics(m.ids, m.cell, cells, col)[0]

    def model_set(m):
        m.stats = new_stats.copy()

    mut = {"append_rows": (lambda i: i.append_rows(ids[sl], coarse_id=t["coarse_id"][sl], codes=t["codes"][sl], vectors=take(vec, sl)),
                           lambda m: m.append(ids[sl], t["coarse_id"][sl], t["codes"][sl], take(vec, sl)), True, 1),
           "remove_rows": (lambda i: i.remove_rows(gone), lambda m: m.remove(gone), True, 2),
           "update_rows": (lambda i: i.update_rows(ids[rows], coarse_id=t["coarse_id"][src], codes=t["codes"][src], vectors=take(vec, src)),
                           lambda m: m.update(ids[rows], t["coarse_id"][src], t["codes"][src], take(vec, src)), False, 3),
           # update_codebook on an ivpq handle overwrites cbT in place and set_statistics d_stats: neither allocates (floor 0, an empty sweep)
           "update_codebook": (lambda i: i.update_codebook(cb2), lambda m: m.update_codebook(cb2), True, None),
           "set_statistics": (lambda i: i.set_statistics(new_stats), model_set, True, None),
           # join.hip create_statistics: the JW_STAT workspace (join_buf) and the pinned staging block h_stat
           "create_statistics": (lambda i: i.create_statistics(col, install=True), model_create, True, None)}[call]
    floor = IVPQ_FLOORS[with_vectors][mut[3]] if mut[3] is not None else (2 if call == "create_statistics" else 0)
    # scratch a failed create_statistics legitimately keeps: JoinIndex::w[JW_STAT] (join_index.h join_buf: grown on demand and kept between
    # calls; allocated before the staging block whose allocation then fails): bytes + bytes / 4 + 256 of 8 * (cells + (cells + 1) / 2 + 1)
    jw = 8 * (cells + (cells + 1) // 2 + 1)
    kept = ((1, jw + jw // 4 + 256),) if call == "create_statistics" else ()
    _sweep_mutation(gpu, oracle, f"ivpq vectors={with_vectors} {call}", kind, make, mut[0], mut[1], floor, mut[2], kept)


MANY = 1100   # rows of the large append: more than an eighth of either table, the headroom the fragment copy is allocated with


def _vec_setup(gpu, shape):
    d, n0 = VEC_SHAPES[shape]
    x, ids = _vec_table(d, n0 + MANY)
    kind = _vec_kind(gpu, x, ids, d, n0)
    return kind, (lambda: um.VecModel(ids[:n0], x[:n0])), x, ids, n0


@pytest.mark.parametrize("shape", list(VEC_SHAPES))
def test_pin_vectors(gpu, helpers, shape):
    kind, make, *_ = _vec_setup(gpu, shape)
    _sweep_pin(gpu, f"pin_vectors {shape}", gpu.VectorIndex, make().pin_args(), {}, VEC_FLOORS[shape][0])


@pytest.mark.parametrize("call", ["append_rows", "append_many", "remove_rows", "update_rows"])
@pytest.mark.parametrize("shape", list(VEC_SHAPES))
def test_vec_mutation(gpu, helpers, oracle, shape, call):
    """append_rows / remove_rows build the three arrays beside the old ones (intact), then the exact filter's statistics and
    fragment copy are rewritten in place (exf_table_stats): a failure there poisons.  65 appended rows fit the headroom of the
    fragment copy (a DevBuf: need + need / 8 + 256 bytes), so that step allocates nothing; 1100 rows do not, and at d = 300, where the
    filter exists, the copy grows: a fourth allocation, AFTER the rows are in -- the one failure of an append that poisons.
    update_rows writes in place throughout."""
    kind, make, x, ids, n0 = _vec_setup(gpu, shape)
    rng = np.random.default_rng(n0 + 2)
    gone = np.concatenate([ids[rng.choice(n0, 70, replace=False)], [4, 10 ** 8]]).astype(np.int32)
    rows, src = rng.choice(n0, 40, replace=False), rng.choice(n0, 40, replace=False)
    sl = slice(n0, n0 + 65)
    big = slice(n0, n0 + MANY)
    mut = {"append_rows": (lambda i: i.append_rows(ids[sl], vectors=x[sl]), lambda m: m.append(ids[sl], x[sl]), 1),
           "append_many": (lambda i: i.append_rows(ids[big], vectors=x[big]), lambda m: m.append(ids[big], x[big]), 1),
           "remove_rows": (lambda i: i.remove_rows(gone), lambda m: m.remove(gone), 2),
           "update_rows": (lambda i: i.update_rows(ids[rows], vectors=x[src]), lambda m: m.update(ids[rows], x[src]), 3)}[call]
    states = _sweep_mutation(gpu, oracle, f"vec {shape} {call}", kind, make, mut[0], mut[1], VEC_FLOORS[shape][mut[2]], False)
    if call != "update_rows":
        assert states[:3] == ["I"] * 3, states           # the arrays built beside the old ones
    if call == "append_many":                            # + the larger fragment copy where the shape has the filter (exact.hip exf_table_stats)
        assert states == (["I"] * 3 + ["P"] if shape == "d300" else ["I"] * 3), states
