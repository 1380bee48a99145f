"""Inputs for the edge tests of option assign_filter (csrc/assign_filter.h), and what follows from them ALONE: the documented bracket
eps(x) = asf_eps_rel(d) |x| max|q| + 2e-34 in fp64, the scale exponents as the kernels derive them, and predicted_redo(), the set of
targets the filter has to send to the all-exact walk.  tests/test_assign_filter_inputs_cpu.py proves, without a GPU, every property
the GPU suite (tests/test_gpu_assign_filter_edges.py) builds an exact expectation on.

The redo rule.  The filter keeps a centroid when a + eps >= L, L = (largest a so far) - eps, |a - s| <= eps: a centroid whose fp64
similarity s is more than 4 eps below the prefix maximum is never on a list, one that EQUALS it always is.  So where, at every tile
boundary b, every similarity of [0, b) either equals the prefix maximum or lies >= 8 eps below it (top_separated: the part of "any two
distinct values differ by 8 eps" the argument uses -- a thousand random centroids cannot be pairwise separated), the list at b holds
exactly the copies of the prefix maximum, plus stale entries of earlier maxima that a compaction removes whenever the list passes
ENC_KEEP; carried (<= 16) + arrivals pass ENC_CAP only when the new plateau alone passes 16.  Redo <=> some prefix plateau > 16, or
a non-finite / scale condition (scale_redo).

Where the documented eps does NOT determine the redo set.  csrc/assign_filter.h documents eps(x) = asf_eps_rel(d) xn max|q| + ENC_EPS_ABS
with "xn >= |x|" (the lines "xn >= |x|: the kernel's own |x|^2 ..." and "... below the 2^-69 that is added to the root" of its header
comment; `const float xn = __builtin_sqrtf(n2) * (1.0f + 1e-5f) + 0x1p-69f` in assign_filter_kernel).  For a row whose |x| is far below
2^-69 the kernel's eps is therefore orders of magnitude above eps_rel |x| max|q| + 2e-34: every centroid lies inside its bracket, and
with more than 16 centroids the target is redone although predicted_redo(), which knows the documented eps only, says it is not.
max|q| is kept as a binary32 as well: above binary32's range eps is infinite (scale_redo models that).  scale_cases() therefore stays
at Q = 16, where no list can pass ENC_KEEP; a scale-edge row together with a longer list is NOT covered by an exact prediction.

encode_cases(): the same list mechanics in csrc/encode_filter.h, with "minimum distance" in place of "maximum similarity" and the
bracket enc_eps_rel(S) (|x| + max|c|)^2 + 2e-34."""
import functools

import numpy as np

import assign_model as am

KEEP, TILE = 16, 128                   # csrc/encode_filter.h ENC_KEEP (ENC_CAP = 32 = 16 carried + 16 new); centroids per streamed tile
MAX_EXP = 120                          # csrc/encode_filter.h ENC_MAX_EXP
EPS_ABS = 2e-34                        # csrc/encode_filter.h ENC_EPS_ABS
AS_PASS = 1 << 22                      # csrc/cluster.hip AS_PASS
ASF_ALL_BYTES = 512 << 20              # csrc/assign_filter.h ASF_ALL_BYTES
F32_MAX = float(np.finfo(np.float32).max)


def eps_rel(d):                        # csrc/assign_filter.h asf_eps_rel
    return 2.5e-5 if d <= 64 else 9e-5 if d <= 320 else 1.4e-4


def check_pass(Q):                     # csrc/assign_filter.h asf_check_pass
    return max(64, ASF_ALL_BYTES // (4 * ((Q + TILE - 1) // TILE * TILE)))


def eps_of(rows, qs):
    """eps(x) per row as the header documents it, fp64."""
    x, q = np.asarray(rows, np.float64), np.asarray(qs, np.float64)
    with np.errstate(all="ignore"):
        return eps_rel(x.shape[1]) * np.linalg.norm(x, axis=1) * np.linalg.norm(q, axis=1).max() + EPS_ABS


def sims64(rows, qs):
    """[n][Q] fp64 similarities; copies of one centroid vector get the SAME number (computed once per distinct vector)."""
    q = np.ascontiguousarray(qs, np.float32)
    uq, inv = np.unique(q.view(np.uint32), axis=0, return_inverse=True)
    with np.errstate(all="ignore"):
        return (np.asarray(rows, np.float64) @ uq.view(np.float32).astype(np.float64).T)[:, np.asarray(inv).reshape(-1)]


def boundaries(Q):
    return list(range(TILE, Q, TILE)) + [Q]


def crowded(rows, qs):
    """tests/test_gpu_assign_filter.py's rule: may more than KEEP centroids lie inside the bracket (4 eps) at some tile boundary?"""
    s, eps = sims64(rows, qs), eps_of(rows, qs)
    out = np.zeros(len(s), bool)
    for b in boundaries(s.shape[1]):
        out |= (s[:, :b] >= s[:, :b].max(axis=1, keepdims=True) - 4 * eps[:, None]).sum(axis=1) > KEEP
    return out


def top_separated(rows, qs, k=8.0):
    """Per row: at every tile boundary every similarity of the prefix equals the prefix maximum or lies >= k eps below it."""
    s, eps = sims64(rows, qs), eps_of(rows, qs)
    ok = np.ones(len(s), bool)
    for b in boundaries(s.shape[1]):
        m = s[:, :b].max(axis=1, keepdims=True)
        ok &= ((s[:, :b] == m) | (s[:, :b] <= m - k * eps[:, None])).all(axis=1)
    return ok


def scale_exp(amax):
    """14 - exponent(amax) with frexp's exponent (amax = f * 2^exponent, 0.5 <= f < 1), 0 for amax = 0: the e of a row, the ec of a set
    of centroids (assign_filter_kernel / assign_image_kernel).  A binary32 has exponent <= 128: no e below -114 exists."""
    amax = np.asarray(amax, np.float64)
    return np.where(amax > 0, 14 - np.frexp(np.where(amax > 0, amax, 1.0))[1], 0).astype(np.int64)


def image_flag(qs):
    """(flag, ec): the image's flag -- a non-finite centroid element or a centroid scale outside [-MAX_EXP, MAX_EXP] -- and ec."""
    q = np.asarray(qs, np.float32)
    if not np.isfinite(q).all():
        return True, 0
    ec = int(scale_exp(np.abs(q).max() if q.size else 0.0))
    return (ec < -MAX_EXP or ec > MAX_EXP), ec


def scale_redo(rows, qs):
    """Per row: the non-finite and scale conditions of the header's list.  |x|^2 and eps are taken in fp64 here; margin_ok() says
    whether they are far enough from binary32's overflow and from 1e30 for that to decide what the kernel's fp32 decides."""
    x = np.asarray(rows, np.float32)
    flag, ec = image_flag(qs)
    if flag:
        return np.ones(len(x), bool)
    if np.linalg.norm(np.asarray(qs, np.float64), axis=1).max() >= F32_MAX:    # max|q| is kept as a binary32: eps is infinite
        return np.ones(len(x), bool)
    fin = np.isfinite(x).all(axis=1)
    xz = np.where(fin[:, None], x, 0).astype(np.float64)
    e = scale_exp(np.abs(xz).max(axis=1))
    n2 = (xz * xz).sum(axis=1)
    bad = ~fin | (np.abs(e) > MAX_EXP) | (np.abs(e + ec) > MAX_EXP) | (n2 >= F32_MAX) | (eps_of(xz, qs) >= 1e30)
    return bad


def margin_ok(rows, qs):
    """Every finite row's |x|^2 and the largest |q| are a factor 2 away from binary32's largest number, every eps a factor 4 from 1e30."""
    x = np.asarray(rows, np.float32)
    xz = x[np.isfinite(x).all(axis=1)].astype(np.float64)
    n2, eps = (xz * xz).sum(axis=1), eps_of(xz, qs)
    cm = np.linalg.norm(np.asarray(qs, np.float64), axis=1).max()
    return bool((cm < F32_MAX / 2 or cm > F32_MAX * 2) and (((n2 < F32_MAX / 2) | (n2 > F32_MAX * 2)) & ((eps < 1e30 / 4) | (eps > 4e30))).all())


def predicted_redo(rows, qs):
    """Per row (a target WITH a row): does the filter send it to the redo?  Needs top_separated (or at most KEEP centroids)."""
    s = sims64(rows, qs)
    out = scale_redo(rows, qs)
    with np.errstate(all="ignore"):
        for b in boundaries(s.shape[1]):
            out = out | ((s[:, :b] == s[:, :b].max(axis=1, keepdims=True)).sum(axis=1) > KEEP)
    return out


def target_rows(ids, x, tg):
    """(have, rows of the targets that have one)"""
    r = am.rows_of(ids, tg)
    return r >= 0, np.asarray(x)[r[r >= 0]]


# =======================================================================================
# A. the bracket under pressure
# =======================================================================================
GAPS = (0.0, 1e-3, 0.5, 1.5, 3.0, 6.0)                       # eps below the group's q_0
BINS = ((0.0, 0.01), (0.0, 0.01), (0.3, 0.7), (1.2, 1.8), (2.5, 3.5), (5.0, 7.0))   # of (group maximum - s) / eps, after rounding
N_PROBES, Q_TIES = 32, 200
DIMS = (16, 64, 65, 320, 321, 512)     # T = 1 (< ENC_PF k-steps); both sides of asf_eps_rel's edges; d % 4 != 0


def _corpus(d, n, seed, wide):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, min(10, d))) @ rng.standard_normal((min(10, d), d)) + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    if wide:                            # elements spanning 2^-12 .. 1 around the largest: lo halves that are subnormal in f16
        x = x * np.exp2(-rng.integers(0, 13, d)).astype(np.float32)
        x[:, rng.integers(0, d)] *= np.float32(4.0)
    return x


def _nudge(q, x, s_goal):
    """Move single elements of the binary32 vector q by one ulp at a time until x.q (fp64) is within 2e-4 |steps available| of s_goal."""
    q = q.copy()
    x64 = x.astype(np.float64)
    for _ in range(200):
        err = float(x64 @ q.astype(np.float64)) - s_goal
        up, dn = np.nextafter(q, np.float32(np.inf)), np.nextafter(q, np.float32(-np.inf))
        step = np.where(x64 * err > 0, dn, up).astype(np.float32)          # the neighbour that moves x.q towards the goal
        eff = np.abs(x64 * (step.astype(np.float64) - q.astype(np.float64)))
        ok = (eff > 0) & (eff <= abs(err))
        if not ok.any():
            break
        j = int(np.argmax(np.where(ok, eff, 0)))
        q[j] = step[j]
    return q


@functools.lru_cache(maxsize=None)
def near_ties(d, wide=False):
    """(x, ids, qs, tg, probes, groups): a table of 300 rows, N_PROBES probe rows with a group of 6 centroids each, q_k = q_0 -
    GAPS[k] eps x / |x|^2 rounded to binary32 (the 1e-3 one nudged by single ulps), q_0 = x scaled to the largest background norm,
    8 background centroids (means of 10 rows), all 200 in a fixed random order; the targets are every id and ids without a row."""
    n0 = 300
    x = _corpus(d, n0, 500 + d + 7 * wide, wide)
    ids = np.arange(1, n0 + 1, dtype=np.int32)
    rng = np.random.default_rng(900 + d + wide)
    bg = np.stack([x[rng.choice(n0, 10)].mean(axis=0) for _ in range(Q_TIES - 6 * N_PROBES)]).astype(np.float32)
    xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    probes = []
    for r in rng.permutation(n0):       # probe rows no two of which point the same way
        if all(abs(float(xn[r] @ xn[p])) < 0.9 for p in probes):
            probes.append(int(r))
        if len(probes) == N_PROBES:
            break
    assert len(probes) == N_PROBES
    M = float(np.linalg.norm(bg.astype(np.float64), axis=1).max()) * 1.05
    qs = np.zeros((Q_TIES, d), np.float32)
    order = rng.permutation(Q_TIES)
    groups = np.zeros((N_PROBES, 6), np.int64)
    qs[order[6 * N_PROBES:]] = bg
    for p, r in enumerate(probes):
        x64 = x[r].astype(np.float64)
        q0 = (xn[r] * M).astype(np.float32)
        eps = eps_rel(d) * np.linalg.norm(x64) * M * 1.0001 + EPS_ABS
        s0 = float(x64 @ q0.astype(np.float64))
        for k, g in enumerate(GAPS):
            qk = q0 if k == 0 else (q0.astype(np.float64) - g * eps * x64 / (x64 @ x64)).astype(np.float32)
            if k == 1:
                qk = _nudge(qk, x[r], s0 - g * eps)
            groups[p, k] = order[6 * p + k]
            qs[groups[p, k]] = qk
    tg = np.concatenate([ids, [n0 + 5, -3]]).astype(np.int32)
    return x, ids, qs, tg, np.array(probes), groups


@functools.lru_cache(maxsize=None)
def cancellation(d):
    """Targets nearly orthogonal to every centroid: x = (v, -v) + t, q = (u, u), u and v positive -- x.q = t.q, a few eps with both
    signs, while sum |x_j q_j| ~ 2 v.u is close to |x||q|.  12 centroids: a list never passes KEEP."""
    rng = np.random.default_rng(40 + d)
    h, n0, Q = d // 2, 70, 12
    u = (1.0 + 0.05 * rng.random((Q, h))).astype(np.float32)
    v = (1.0 + 0.05 * rng.random((n0, h))).astype(np.float32)
    qs, x = np.zeros((Q, d), np.float32), np.zeros((n0, d), np.float32)
    qs[:, :h], qs[:, h:2 * h] = u, u
    x[:, :h], x[:, h:2 * h] = v, -v
    t = rng.standard_normal((n0, d)) * (3 * eps_rel(d) / np.sqrt(d))
    x = (x.astype(np.float64) + t).astype(np.float32)
    ids = np.arange(1, n0 + 1, dtype=np.int32)
    return x, ids, qs, ids.copy()


@functools.lru_cache(maxsize=None)
def all_negative(d, Q):
    """Rows with all elements positive, centroids with all elements negative: every real similarity is below the 0 of a padded one."""
    rng = np.random.default_rng(60 + d + Q)
    x = (0.1 + rng.random((90, d))).astype(np.float32)
    qs = (-0.1 - rng.random((Q, d))).astype(np.float32)
    ids = np.arange(1, 91, dtype=np.int32)
    keep = np.flatnonzero(top_separated(x, qs))[:70]       # (the rows the prediction speaks about)
    return x, ids, qs, np.concatenate([ids[keep], [200]]).astype(np.int32)


def zero_cases(d=30):
    """name -> (x, ids, qs, tg, winner of the zero row or None).  Row 3 is all zeros."""
    rng = np.random.default_rng(70)
    x = rng.standard_normal((80, d)).astype(np.float32)
    x[3] = 0
    ids = np.arange(1, 81, dtype=np.int32)
    q = rng.standard_normal((40, d)).astype(np.float32)
    qz = q[:20].copy(); qz[7] = 0
    keep = lambda qs: np.concatenate([[4], ids[np.flatnonzero(top_separated(x, qs) & (np.arange(80) != 3))]]).astype(np.int32)
    return {"zero_row_Q16": (x, ids, q[:16], keep(q[:16]), 0), "zero_row_Q17": (x, ids, q[:17], keep(q[:17]), 0),
            "zero_centroid": (x, ids, qz, keep(qz), 0), "all_zero_centroids": (x, ids, np.zeros((5, d), np.float32), ids.copy(), 0)}


def scale_cases(d=30):
    """name -> (x, ids, qs, tg).  Q = 16: no list can pass KEEP, so the redo set is scale_redo() alone -- the kernel's eps of a tiny row
    is far above the documented one (the 2^-69 added to the root) and crowds every list of more than 16.  Rows 0 .. 5 are scaled so
    that e = 14 - exponent(max |x_j|) lands on 120, 121 (both sides of ENC_MAX_EXP), -114 (the smallest e a binary32 allows: there is
    no -120), and e + ec on +-120 / +-121 for the centroid scales below."""
    rng = np.random.default_rng(80)
    x = rng.standard_normal((70, d)).astype(np.float32)
    base = x.copy()
    ids = np.arange(1, 71, dtype=np.int32)
    q = rng.standard_normal((16, d)).astype(np.float32)

    def scaled(v, e):                   # v times the power of two that makes its scale exponent e
        v = np.asarray(v, np.float32)
        return np.ldexp(v, int(scale_exp(np.abs(v).max())) - e).astype(np.float32)
    out = {}
    xr = base.copy()
    for row, e in ((0, 120), (1, 121), (2, -114), (3, 119), (4, -113)):
        xr[row] = scaled(base[row], e)
    out["rows"] = (xr, ids, scaled(q, 0), ids.copy())       # (ec = 0: e + ec = e)
    for name, ec in (("centroids_120", 120), ("centroids_121", 121), ("centroids_-111", -111), ("centroids_-114", -114)):
        xc = base.copy()
        # rows whose e + ec is at, beyond and inside the range (every other row is beyond it, or its eps is: |x| max|q| >= 2^(26 - e - ec),
        # so a sum below about -85 is always answered by "eps < 1e30" first -- the lower edge of the sum cannot be met alone)
        e_of = {120: (0, 1, -1, -40), 121: (0,), -111: (100, 20), -114: (100,)}[ec]      # (at -114 max|q| is above binary32's range)
        for row, e in enumerate(e_of):
            xc[row] = scaled(base[row], e)
        qc = scaled(q, ec)
        if ec == -114:                  # (one centroid with every element at the largest: |q| clearly above binary32's range)
            qc[0] = np.abs(qc).max()
        out[name] = (xc, ids, qc, ids.copy())
    xs = base.copy()
    for row, e in ((0, 60), (1, 61), (2, 59)):
        xs[row] = scaled(base[row], e)
    out["sum_120_121"] = (xs, ids, scaled(q, 60), ids[:3].copy())
    xs = base.copy()
    for row, e in ((0, -60), (1, -61), (2, -59)):
        xs[row] = scaled(base[row], e)
    out["sum_-120_-121"] = (xs, ids, scaled(q, -60), ids[:3].copy())
    return out


# =======================================================================================
# B. list mechanics over three and more tiles
# =======================================================================================
B_D, B_N = 30, 130                      # two full workgroups of 64 targets and a tail of two
B_QS = (257, 300, 384, 385, 1000)
HANDFUL = (3, 70, 129)                  # positions of the planted row's targets: one in every workgroup


@functools.lru_cache(maxsize=None)
def _b_table():
    rng = np.random.default_rng(11)
    return rng.standard_normal((600, B_D)).astype(np.float32), np.arange(1, 601, dtype=np.int32)


def _b_case(Q, plants, n_planted=None, where=HANDFUL, seed=0):
    """Q random background centroids, then plants: (row, positions, level) puts copies of x[row] scaled to level * (largest background
    norm) there -- level 1 wins row's targets by far, 0.9 is a runner-up.  Targets: the FIRST plant's row at `where` (or at n_planted
    positions from where[0] on), every other position a distinct row that is top_separated against these centroids."""
    x, ids = _b_table()
    rng = np.random.default_rng(1000 + Q + seed)
    qs = rng.standard_normal((Q, B_D)).astype(np.float32)
    M = float(np.linalg.norm(qs.astype(np.float64), axis=1).max())
    for row, pos, level in plants:
        x64 = x[row].astype(np.float64)
        qs[np.asarray(pos)] = (x64 / np.linalg.norm(x64) * M * level).astype(np.float32)
    planted = {row for row, _, _ in plants}
    ok = top_separated(x, qs) & ~predicted_redo(x, qs)     # (a planted plateau may be another row's prefix maximum: not a filler)
    fill = [r for r in range(len(x)) if ok[r] and r not in planted]
    pos = list(where) if n_planted is None else list(range(where[0], where[0] + n_planted))
    tg = np.zeros(B_N, np.int32)
    tg[:] = ids[fill[:B_N]]
    tg[pos] = ids[plants[0][0]]
    tg[1] = 9999                         # an id without a row
    return x, ids, qs, tg, np.array(pos)


def list_cases(Q):
    """name -> (x, ids, qs, tg, positions of the planted targets, their expected winner, are they redone)."""
    last0 = (Q - 1) // TILE * TILE      # first centroid of the last tile
    R, R2 = 7, 8
    r = lambda a, n: list(range(a, a + n))
    out = {}
    singles = [(20 + i, [c], 1.0) for i, c in enumerate(dict.fromkeys((0, 127, 128, 255, 256, Q - 1)))]
    x, ids, qs, tg, _ = _b_case(Q, singles)
    pos = np.arange(10, 10 + len(singles))
    tg[pos] = ids[[p[0] for p in singles]]
    out["single_winners"] = (x, ids, qs, tg, pos, np.array([p[1][0] for p in singles]), False)
    t2 = r(256, 6) if Q >= 262 else r(200, 5) + [256]   # (Q = 257 has one centroid in tile 2: 6 + 10, then the 17th there)
    plans = {"16_in_tile0": ([(R, r(5, 16), 1.0)], 5, False), "17_in_tile0": ([(R, r(5, 17), 1.0)], 5, True),
             "spread_6_5_5": ([(R, r(100, 6) + r(130, 5) + t2[:5], 1.0)], 100, False),
             "spread_6_5_6": ([(R, r(100, 6) + r(130, 5) + t2, 1.0)], 100, True),
             "compaction_12_then_10": ([(R, r(3, 12), 0.9), (R, r(140, 10), 1.0)], 140, False),
             "better_10_then_12": ([(R, r(3, 10), 1.0), (R, r(140, 12), 0.9)], 3, False),
             "16_stale_16_new": ([(R, r(3, 16), 0.9), (R, r(140, 16), 1.0)], 140, False),
             "33_in_one_tile": ([(R, r(40, 33), 1.0)], 40, True)}
    if Q - last0 >= 17:                 # (Q = 257 and 385 have one centroid in their last tile)
        plans["16_in_last_tile"] = ([(R, r(Q - 16, 16), 1.0)], Q - 16, False)
        plans["17_in_last_tile"] = ([(R, r(Q - 17, 17), 1.0)], Q - 17, True)
    for name, (plants, winner, redone) in plans.items():
        x, ids, qs, tg, pos = _b_case(Q, plants)
        out[name] = (x, ids, qs, tg, pos, np.full(len(pos), winner), redone)
    for cnt, first in ((63, 2), (64, 2), (65, 2), (128, 2), (63, 64)):   # (63 from 64 on: every redone target in the second workgroup)
        x, ids, qs, tg, pos = _b_case(Q, [(R2, r(129, 17), 1.0)], n_planted=cnt, where=(first,), seed=cnt)
        out[f"redo_{cnt}_from_{first}"] = (x, ids, qs, tg, pos, np.full(cnt, 129), True)
    return out


# =======================================================================================
# C. passes
# =======================================================================================
@functools.lru_cache(maxsize=None)
def pass_case(n, n_bad_first, n_bad_second, first_pass):
    """(x, ids, qs, tg): about 1500 rows of d = 30 (four of them with a NaN, +Inf, -Inf, both), Q = 17, n targets drawn with
    replacement; ids without a row in both passes; the bad rows are targeted by n_bad_first positions below first_pass and by
    n_bad_second from there on, and by no other."""
    rng = np.random.default_rng(5)
    d, Q = 30, 17
    qs = rng.standard_normal((Q, d)).astype(np.float32)
    x = rng.standard_normal((4000, d)).astype(np.float32)
    x = x[top_separated(x, qs)][:1500]
    bad = np.array([10, 700, 701, 1400])
    x[10, 4] = np.nan; x[700, 0] = np.inf; x[701, d - 1] = -np.inf; x[1400, 2] = np.inf; x[1400, 3] = -np.inf
    ids = (2 * np.arange(1, len(x) + 1)).astype(np.int32)                  # (odd ids have no row)
    good = np.setdiff1d(np.arange(len(x)), bad)
    tg = ids[good[rng.integers(0, good.size, n)]]
    tg[rng.integers(0, n, 1000)] = 7
    tg[[5, first_pass - 1, first_pass, n - 1]] = (-1, 3, 2 ** 31 - 1, 5)
    at = np.concatenate([rng.choice(np.arange(6, first_pass - 1), n_bad_first, replace=False),
                         first_pass + 1 + rng.choice(n - first_pass - 2, n_bad_second, replace=False)])
    tg[at] = ids[bad[np.arange(at.size) % 4]]
    return x, ids, qs, tg.astype(np.int32)


def model_by_id(ids, x, qs, tg):
    """assign_model.exact_assign, evaluated once per distinct id and gathered."""
    u, inv = np.unique(tg, return_inverse=True)
    q, s = am.exact_assign(ids, x, qs, u)
    return q[inv], s[inv]


# =======================================================================================
# D. whole k-means
# =======================================================================================
@functools.lru_cache(maxsize=None)
def three_vector_tokens(d=300, n=500, kc=40):
    """(x, ids, tokens, kc, draws): every token's row is one of 3 vectors.  The pigeonhole gives 14 identical initial centroids of 40
    (40 > 3 * 13), three short of a redo: that one vector holds more than 16 of them, and wins targets, is shown from these draws."""
    rng = np.random.default_rng(21)
    v = rng.standard_normal((3, d)).astype(np.float32)
    x = v[rng.integers(0, 3, 1000)]
    ids = np.arange(1, 1001, dtype=np.int32)
    return x, ids, np.sort(rng.choice(ids, n, replace=False)).astype(np.int32), kc, rng.random(kc + 10 * kc * 9)


@functools.lru_cache(maxsize=None)
def nan_tokens(seed, d=300, n=400, kc=7):
    """(x, ids, tokens, kc, draws): tokens that include a row with a NaN, one with +Inf and one with -Inf."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((600, d)).astype(np.float32)
    x[5, 7] = np.nan; x[300, 0] = np.inf; x[301, d - 1] = -np.inf
    ids = np.arange(1, 601, dtype=np.int32)
    tokens = np.sort(np.union1d(rng.choice(ids, n - 3, replace=False), [6, 301, 302])).astype(np.int32)
    return x, ids, tokens, kc, rng.random(kc + 10 * kc * 9)


NAN_SEED = 2                            # test_assign_filter_inputs_cpu.py: both kinds of round occur in the model's run of this seed


def rounds_flagged(x, ids, tokens, kc, draws, rounds=10):
    """Per round of the model's k-means (tests/cluster_model.py): is a centroid of that round's assignment non-finite (image_flag)?"""
    import cluster_model as cm
    flags = []

    def assign(c):
        flags.append(image_flag(c)[0])
        return am.exact_assign(ids, x, c, tokens)
    cm.cluster(assign, cm.token_vectors(ids, x, tokens), kc, draws, rounds)
    return flags


# =======================================================================================
# G. the same list mechanics in encode_rows (csrc/encode_filter.h)
# =======================================================================================
ENC_D, ENC_M, ENC_K, ENC_POS = 24, 6, 300, 2     # S = 4, three tiles of centroids (the last one holds 44), flat PQ; the planted position
ENC_NEAR = (0, 3, 63, 64, 69)                    # rows put next to the planted centroid: both workgroups of 64 rows


def enc_eps_rel(S):                    # csrc/encode_filter.h enc_eps_rel
    return 2e-5 if S <= 64 else 1.2e-4 if S <= 320 else 2e-4


def enc_dists(xs, cent):
    """([n][K] fp64 |x - c|^2, eps per row): copies of one centroid get the SAME number; eps = enc_eps_rel(S) (|x| + max|c|)^2 + 2e-34."""
    c = np.ascontiguousarray(cent, np.float32)
    uc, inv = np.unique(c.view(np.uint32), axis=0, return_inverse=True)
    x64, c64 = np.asarray(xs, np.float64), uc.view(np.float32).astype(np.float64)
    D = ((x64[:, None, :] - c64[None, :, :]) ** 2).sum(axis=2)[:, np.asarray(inv).reshape(-1)]
    eps = enc_eps_rel(x64.shape[1]) * (np.linalg.norm(x64, axis=1) + np.linalg.norm(c64, axis=1).max()) ** 2 + EPS_ABS
    return D, eps


def enc_separated(xs, cent, k=8.0):
    """Per row: at every tile boundary every distance of the prefix equals the prefix minimum or lies >= k eps above it."""
    D, eps = enc_dists(xs, cent)
    ok = np.ones(len(D), bool)
    for b in boundaries(D.shape[1]):
        m = D[:, :b].min(axis=1, keepdims=True)
        ok &= ((D[:, :b] == m) | (D[:, :b] >= m + k * eps[:, None])).all(axis=1)
    return ok


def enc_predicted_redo(xs, cent):
    """predicted_redo's rule for one position of encode_rows (finite inputs of ordinary magnitude): some prefix plateau of the minimum > KEEP."""
    D, _ = enc_dists(xs, cent)
    out = np.zeros(len(D), bool)
    for b in boundaries(D.shape[1]):
        out |= (D[:, :b] == D[:, :b].min(axis=1, keepdims=True)).sum(axis=1) > KEEP
    return out


@functools.lru_cache(maxsize=None)
def encode_cases():
    """name -> (x [70][24], codebook [6][300][4], first index of the winning copies, are the ENC_NEAR items redone).  Gaussian rows and
    centroids; in position ENC_POS copies of the point P = (6, 6, 6, 6), far from every Gaussian, and the sub-vectors of the
    ENC_NEAR rows next to P; the farther plateau of the compaction case is P + 0.5 (distance 1, above 8 brackets of about 0.012).
    The rows are the first 70 of a seeded stream whose six sub-vectors are all enc_separated against the case's codebook."""
    S = ENC_D // ENC_M
    r = lambda a, n: list(range(a, a + n))
    plans = {"16_in_tile0": ([(r(10, 16), 0.0)], 10, False), "17_in_tile0": ([(r(10, 17), 0.0)], 10, True),
             "16_in_last_tile": ([(r(284, 16), 0.0)], 284, False), "17_in_last_tile": ([(r(283, 17), 0.0)], 283, True),
             "compaction_12_then_10": ([(r(3, 12), 0.5), (r(140, 10), 0.0)], 140, False),
             "33_in_one_tile": ([(r(40, 33), 0.0)], 40, True)}
    out = {}
    for i, (name, (plants, winner, redone)) in enumerate(plans.items()):
        rng = np.random.default_rng(300 + i)
        cb = np.ascontiguousarray(rng.standard_normal((ENC_K, ENC_M, S)).astype(np.float32).transpose(1, 0, 2))
        for pos, off in plants:
            cb[ENC_POS, pos] = np.float32(6.0 + off)
        pool = rng.standard_normal((1500, ENC_D)).astype(np.float32)
        ok = np.all([enc_separated(pool[:, p * S:(p + 1) * S], cb[p]) & ~enc_predicted_redo(pool[:, p * S:(p + 1) * S], cb[p]) for p in range(ENC_M)], axis=0)
        x = pool[ok][:70].copy()
        sub = x[list(ENC_NEAR), ENC_POS * S:(ENC_POS + 1) * S]
        x[list(ENC_NEAR), ENC_POS * S:(ENC_POS + 1) * S] = np.float32(6.0) + np.float32(1e-3) * sub
        out[name] = (x, cb, winner, redone)
    return out
