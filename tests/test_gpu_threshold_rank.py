"""The threshold rank on the GPU: the filter + refine kernels cut at the k-th smallest cheap bound (the W-th for the
cell choice), the exact stage keeps 2k (2W) keys.  Built cases in which the difference between the two shows -- ties straddling
the cut, exactly k rows below it, carried lists, tied centroids -- against the oracle, bit for bit, with the four-wave
(scan_share 1) and the one-wave (scan_share 4) plan and merge, and the kernels' own bracket counters at zero.

The tables are built, not trained: a query sits exactly on a centroid plus the codewords h of its group, and codewords planted at a
known offset from h's give rows at known distances -- |offset|^2, whatever the query's noise does to the last bits."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

D, M, S = 300, 12, 25
FILT5_EPS = 512.0 * 2.0 ** -24          # the filter's margin E is at least this x |q|^2 (refine.h filter_width5)


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


class Tables:
    """C cells of the given sizes around one base point, random codes; plant() rewrites rows and codewords."""

    def __init__(self, seed, K, sizes, spread=0.25):
        self.rng = rng = np.random.default_rng(seed)
        self.K, self.C, self.N = K, len(sizes), int(np.sum(sizes))
        self.base = rng.standard_normal(D).astype(np.float32)                 # |q|^2 ~ 300: a margin E of ~1e-2
        self.coarse = (self.base + spread * rng.standard_normal((self.C, D))).astype(np.float32)
        self.codebook = (0.15 * rng.standard_normal((M, K, S))).astype(np.float32)
        self.codes = rng.integers(0, K - 64, size=(self.N, M)).astype(np.int16)   # the last 64 codes of a position: planted
        self.list_off = np.zeros(self.C + 1, np.int32)
        self.list_off[1:] = np.cumsum(sizes)
        self.ids = (np.arange(self.N) * 5 + 3).astype(np.int32)                # (ascending inside a list: the scan order)
        self.free = [list(rng.permutation(np.arange(self.list_off[c], self.list_off[c + 1]))) for c in range(self.C)]
        self.next_code = np.full(M, K - 1)

    def decode(self, codes):
        return np.concatenate([self.codebook[p, codes[p]] for p in range(M)])

    def codeword_at(self, p, near, sq):
        """a new code of position p whose codeword lies at squared distance sq from codeword `near`, always in the same direction"""
        code = int(self.next_code[p])
        self.next_code[p] -= 1
        assert code >= self.K - 64, "out of planted codes"
        u = np.zeros(S)
        u[(3 * p) % S] = 1.0
        self.codebook[p, code] = (self.codebook[p, near].astype(np.float64) + np.sqrt(sq) * u).astype(np.float32)
        return code

    def put(self, cell, rows):
        """rows (code vectors) into free slots of the cell, interleaved in scan order"""
        slots = sorted(self.free[cell].pop() for _ in rows)
        for slot, j in zip(slots, self.rng.permutation(len(rows))):
            self.codes[slot] = rows[j]

    def group(self, cell, k, ties, tie_sq=1.0, above=0):
        """k - 1 rows below tie_sq at distinct distances, `ties` rows AT tie_sq, `above` rows 1e-4, 2e-4, ... above it (less than
        E); returns the residual of the query that sees them at these distances."""
        h = self.rng.integers(0, self.K - 64, size=M).astype(np.int16)
        rows = []
        for i in range(k - 1):
            r = h.copy()
            r[i % M] = self.codeword_at(i % M, h[i % M], 0.01 * (1 + i))
            rows.append(r)
        t = h.copy()
        t[1] = self.codeword_at(1, h[1], tie_sq)
        rows += [t] * ties
        for j in range(above):
            r = h.copy()
            r[j % M] = self.codeword_at(j % M, h[j % M], tie_sq + 1e-4 * (1 + j))
            rows.append(r)
        self.put(cell, rows)
        return self.decode(h)

    def pin(self, gpu, oracle):
        ot = oracle.ivf_table(self.coarse, self.codebook, self.list_off, self.ids, self.codes)
        return ot, gpu.IVFIndex(self.coarse, self.codebook, self.list_off, self.ids, self.codes)


def near(rng, points, copies, noise=1e-3):
    """every point as it is, then `copies - 1` noisy copies of it"""
    out = [points] + [points + noise * rng.standard_normal(points.shape) for _ in range(copies - 1)]
    return np.concatenate(out).astype(np.float32)


def check(idx, oracle, ot, qs, k, W, what, sentinels=(1000.0,), rules=(0, 1), shares=(1, 4)):
    for sent in sentinels:
        for rule in rules:
            exp = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)
            for share in shares:
                idx.set_option("scan_share", share)
                gi, gd = idx.search(qs, k, W, sentinel=sent, found_rule=rule)
                util.assert_same_lists(gi, gd, exp, f"{what}: k={k} W={W} sentinel={sent!r} rule={rule} scan_share={share}")
    assert idx.bound_violations() == 0, f"{what}: a refined row or cell left its proven bracket"


def sizes_of(rng, C, N):
    return np.bincount(rng.integers(0, C, size=N), minlength=C)


KS = (1, 5, 10)
WS = (1, 3)


def build_ties(seed, K):
    """(a): per k, groups whose 2k + 3 tied rows sit at the k-th place, their ids interleaved with those of the rows below"""
    rng = np.random.default_rng(seed)
    t = Tables(seed, K, sizes_of(rng, 7, 6000))
    res = {k: np.stack([t.coarse[c] + t.group(c, k, 2 * k + 3) for c in rng.choice(7, size=3, replace=False)]) for k in KS}
    return t, {k: near(rng, res[k], 11) for k in KS}                        # 33 queries per k (>= 32: the MFMA cell selection)


@pytest.mark.parametrize("K", [1024, 256])
def test_ties_straddling_the_cut(gpu, oracle, K, monkeypatch):
    """(a) 2k + 3 rows share the query's k-th smallest exact distance: k + 2k + 2 rows lie within E of the k-th smallest bound, the
    merge keeps 2k exact keys of them, and the tie is decided by scan order.  A sentinel ON the tied distance rejects them all."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    t, qs = build_ties(31, K)
    ot, idx = t.pin(gpu, oracle)
    for k in KS:
        wide = oracle.ivfadc_search_many(ot, qs[k], 3 * k + 2, 1)["dist"].reshape(len(qs[k]), -1)
        assert np.all(wide[:, k - 1] == wide[:, 3 * k + 1]), "the built tie is not at the k-th place"
        assert k == 1 or np.all(wide[:, k - 2] < wide[:, k - 1])
        for W in WS:
            check(idx, oracle, ot, qs[k], k, W, f"ties K={K}", sentinels=(1000.0, float(wide[0, k - 1])))
    idx.close()


@pytest.mark.parametrize("K", [1024, 256])
def test_exactly_k_rows_below_then_thirty_within_the_margin(gpu, oracle, K, monkeypatch):
    """(b) k rows at or below d*, the next 30 rows less than E above it: every one of them passes T = (k-th smallest bound) + E --
    more than the merge keeps in registers for small k (it revisits the survivors) -- and none of them may enter the list."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    rng = np.random.default_rng(32)
    t = Tables(32, K, sizes_of(rng, 9, 6000))
    res = {k: np.stack([t.coarse[c] + t.group(c, k, 1, above=30) for c in (k % 9, (k + 4) % 9)]) for k in KS}
    ot, idx = t.pin(gpu, oracle)
    for k in KS:
        qs = near(rng, res[k], 16, noise=1e-6)                              # (far less than the rows' steps of 1e-4)
        wide = oracle.ivfadc_search_many(ot, qs, k + 30, 1)["dist"].reshape(len(qs), -1)
        gap = wide[:, k + 29] - wide[:, k - 1]
        assert np.all(wide[:, k] > wide[:, k - 1]) and np.all(gap < FILT5_EPS * np.sum(qs * qs, axis=1)), "the built rows are not within E"
        for W in WS:
            check(idx, oracle, ot, qs, k, W, f"k rows below K={K}", sentinels=(1000.0, float(wide[0, k])))
    idx.close()


TINY = {1: ([0, 0, 0, 0, 0, 0], 0), 5: ([1, 0, 1, 1, 0, 1], 2), 10: ([2, 1, 2, 1, 2, 1], 3)}   # k: rows of its six tiny cells, how many of them near


def build_tiny(seed, K):
    """(c): per k one query point, on a full cell's centroid plus its group's codewords; the six cells nearest to it are tiny (fewer
    than k rows in all), the full cell with the tie group is the seventh.  Some tiny rows lie BELOW the tie (codewords of all zeros:
    the row's distance is the tiny cell's coarse distance, 0.1 .. 0.6), the others far above it: the list carried into the last
    round has fewer than k real entries, some of which stay; with the rows below the tie in the full cell they are k - 1."""
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([np.concatenate([TINY[k][0] for k in KS]), sizes_of(rng, 8, 6000)])
    t = Tables(seed, K, sizes)
    zero = np.array([t.next_code[p] for p in range(M)], np.int16)               # one planted code per position: the zero codeword
    t.next_code -= 1
    for p in range(M):
        t.codebook[p, zero[p]] = 0.0
    points, full = {}, {}
    for i, k in enumerate(KS):
        rows, n_near = TINY[k]
        full[k] = 18 + i
        points[k] = (t.coarse[full[k]] + t.group(full[k], k - n_near, 2 * k + 3)).astype(np.float32)
        for j in range(6):
            c = 6 * i + j
            v = rng.standard_normal(D)
            t.coarse[c] = points[k] + (np.sqrt(0.1 * (j + 1)) * v / np.linalg.norm(v)).astype(np.float32)
        slots = [s for j in range(6) for s in range(t.list_off[6 * i + j], t.list_off[6 * i + j + 1])]
        for s in slots[:n_near]:
            t.codes[s] = zero
    return t, points, full


@pytest.mark.parametrize("K", [1024, 256])
def test_tiny_cells_carry_lists_into_new_ties(gpu, oracle, K, monkeypatch):
    """(c) the 2W cells nearest to every query hold fewer than k rows: found < k sends it into a second and a third round (W = 3; six
    more rounds with W = 1), and the list carried there meets 2k + 3 tied rows at the k-th place.  A sentinel ON the tie as in (a)."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    t, points, full = build_tiny(33, K)
    ot, idx = t.pin(gpu, oracle)
    rows_of = np.diff(t.list_off)
    for i, k in enumerate(KS):
        qs = near(t.rng, points[k][None], 32)
        cd = np.sum((qs[:, None, :].astype(np.float64) - t.coarse[None].astype(np.float64)) ** 2, axis=2)
        order = np.argsort(cd, axis=1)
        assert np.all(np.sort(order[:, :6], axis=1) == 6 * i + np.arange(6)) and np.all(order[:, 6] == full[k]), "the tiny cells are not the nearest six"
        for W in WS:                                                            # (rounds one and two find fewer than k rows, for every query)
            assert np.all(rows_of[order[:, :W]].sum(axis=1) < k) and np.all(rows_of[order[:, :2 * W]].sum(axis=1) < k)
        wide = oracle.ivfadc_search_many(ot, qs, 3 * k + 2, 3)["dist"].reshape(len(qs), -1)
        assert np.all(wide[:, k - 1] == wide[:, 3 * k + 1]), "the built tie is not at the k-th place"
        assert k == 1 or np.all(wide[:, k - 2] < wide[:, k - 1])
        for W in WS:
            check(idx, oracle, ot, qs, k, W, f"tiny cells K={K}", sentinels=(1000.0, float(wide[0, k - 1])))
    idx.close()


def build_cell_ties(seed, W, C, N):
    """(d): W - 1 centroids near every query, then W + 2 IDENTICAL ones, two more within 2 eps of those, the rest far; at random
    cell ids"""
    rng = np.random.default_rng(seed)
    t = Tables(seed, 256, sizes_of(rng, C, N), spread=0.5)
    cells = rng.permutation(C)
    near_c, dup_c, close_c = cells[:W - 1], cells[W - 1:2 * W + 1], cells[2 * W + 1:2 * W + 3]
    for i, c in enumerate(near_c):
        t.coarse[c] = t.base + (0.05 * (i + 1) / W * rng.standard_normal(D)).astype(np.float32)
    dup = t.base + (0.2 * rng.standard_normal(D)).astype(np.float32)
    t.coarse[dup_c] = dup
    for c in close_c:                     # |q - dup| ~ 3.5: the distance moves by < 0.08, 2 eps = 2 * 1.2e-4 (|q| + max |c|)^2 ~ 0.29
        v = rng.standard_normal(D)
        t.coarse[c] = dup + (0.01 * v / np.linalg.norm(v)).astype(np.float32)
    qs = (t.base + 0.1 * rng.standard_normal((64, D))).astype(np.float32)
    return t, qs, dup_c


@pytest.mark.parametrize("W,C", [(1, 16), (4, 16), (10, 28), (4, 1100)])
def test_cell_choice_ties_at_the_wth_place(gpu, oracle, W, C, monkeypatch):
    """(d) W + 2 identical centroids at the W-th place of every query's cell order and two more cells within 2 eps: the candidates
    of the plan's exact stage, cut at the W-th smallest approximate distance; 1100 cells: the streamed two-level plan."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    t, qs, dup_c = build_cell_ties(40 + W + C, W, C, 6000)
    ot, idx = t.pin(gpu, oracle)
    cd = np.sum((qs[:, None, :].astype(np.float64) - t.coarse[None].astype(np.float64)) ** 2, axis=2)
    assert np.all(np.sum(cd < cd[:, dup_c[:1]] - 1.0, axis=1) == W - 1), "the tied centroids are not at the W-th place"
    check(idx, oracle, ot, qs, 5, W, f"cell ties C={C}")
    idx.close()


def test_every_bracket_checked(gpu, oracle, monkeypatch):
    """(e) check_brackets 1: every probed row goes through the exact stage; 2: every cell does.  No distance outside its bracket."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    t, qs = build_ties(31, 256)
    ot, idx = t.pin(gpu, oracle)
    for mode in (1, 2):
        idx.set_option("check_brackets", mode)
        before = idx.bound_checked() + idx.coarse_bound_checked()
        check(idx, oracle, ot, qs[5], 5, 3, f"check_brackets={mode}", rules=(0,), shares=(1,))
        assert idx.bound_checked() + idx.coarse_bound_checked() > before, "nothing was checked"
    idx.close()


@pytest.mark.parametrize("k", [5, 32])
def test_flat_pq_table_ties(gpu, oracle, k):
    """(f) the PARTIAL merge: a batch over the flat PQ table, every slice cut at its own k-th smallest bound."""
    t = Tables(50 + k, 256, [8000])
    res = np.stack([t.group(0, k, 2 * k + 3) for _ in range(4)])
    qs = near(t.rng, res, 16)
    ot = oracle.pq_table(t.codebook, t.ids, t.codes)
    idx = gpu.PQIndex(t.codebook, t.ids, t.codes)
    wide = np.stack([oracle.pq_search(ot, q, 3 * k + 2) for q in qs[:4]])["dist"]
    assert np.all(wide[:, k - 1] == wide[:, 3 * k + 1]), "the built tie is not at the k-th place"
    exp = np.stack([oracle.pq_search(ot, q, k) for q in qs])
    gi, gd = idx.search(qs, k, sentinel=100.0)
    util.assert_same_lists(gi, gd, exp, f"flat PQ table k={k}")
    assert idx.bound_violations() == 0
    idx.close()
