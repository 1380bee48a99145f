"""Plain-Python model of the tables behind a pinned handle under freddy_gpu_append_rows / freddy_gpu_update_codebook
(include/freddy_gpu.h; postgres-word2vec_amd/csrc/mutate.h, pin.hip).

One class per handle kind.  Each holds the HOST arrays, applies a mutation the way the header documents it -- pq, ivpq and
vector rows stay in id order, an ivf row joins the END of its cell's list -- and yields the arrays for a fresh pin
(pin_args) and for the oracle's table constructor.  A call the library refuses (ids that do not ascend beyond the pinned
ones, a cell or a code out of range, a missing array) raises Refused and leaves the model as it was, as the library must
leave the handle."""
import numpy as np


class Refused(ValueError):
    pass


def _check_ids(ids, last_id):
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    prev = np.concatenate([np.array([last_id], np.int64), ids[:-1].astype(np.int64)])
    bad = np.nonzero(ids.astype(np.int64) <= prev)[0]
    if bad.size:
        raise Refused(f"id not ascending at new row {int(bad[0])}")
    return ids


def _check_codes(codes, n, m, K):
    if codes is None:
        raise Refused("codes are required")
    codes = np.ascontiguousarray(codes, np.int16).reshape(n, m)
    bad = np.argwhere((codes < 0) | (codes >= K))
    if bad.size:
        raise Refused(f"code out of range at new row {int(bad[0][0])}")
    return codes


def _check_cells(cell, n, C):
    if cell is None:
        raise Refused("coarse_id is required")
    cell = np.ascontiguousarray(cell, np.int32).reshape(n)
    bad = np.nonzero((cell < 0) | (cell >= C))[0]
    if bad.size:
        raise Refused(f"coarse_id out of range at new row {int(bad[0])}")
    return cell


def _check_codebook(old, new):
    if new is None:
        raise Refused("codebook is required")
    new = np.ascontiguousarray(new, np.float32)
    assert new.shape == old.shape
    return new.copy()


class PQModel:
    """pq_codebook + pq_quantization: rows in id order."""

    def __init__(self, codebook, ids, codes):
        self.codebook = np.ascontiguousarray(codebook, np.float32).copy()
        self.m, self.K, _ = self.codebook.shape
        self.ids = np.ascontiguousarray(ids, np.int32).copy()
        self.codes = np.ascontiguousarray(codes, np.int16).reshape(self.ids.size, self.m).copy()

    @property
    def N(self):
        return self.ids.size

    def append(self, ids, codes=None):
        ids = _check_ids(ids, self.ids[-1] if self.N else -1)
        codes = _check_codes(codes, ids.size, self.m, self.K)
        self.ids = np.concatenate([self.ids, ids])
        self.codes = np.concatenate([self.codes, codes])

    def update_codebook(self, codebook):
        self.codebook = _check_codebook(self.codebook, codebook)

    def pin_args(self):
        return self.codebook, self.ids, self.codes

    def oracle_table(self, oracle):
        return oracle.pq_table(*self.pin_args())


class IVFModel:
    """coarse_quantization + residual_codebook + fine_quantization: one list of (id, codes) per cell, a new row at its end."""

    def __init__(self, coarse, codebook, list_off, ids, codes):
        self.coarse = np.ascontiguousarray(coarse, np.float32).copy()
        self.codebook = np.ascontiguousarray(codebook, np.float32).copy()
        self.m, self.K, _ = self.codebook.shape
        self.C = self.coarse.shape[0]
        lo = np.asarray(list_off, np.int64)
        ids = np.ascontiguousarray(ids, np.int32)
        codes = np.ascontiguousarray(codes, np.int16).reshape(ids.size, self.m)
        self.list_ids = [ids[lo[c]:lo[c + 1]].copy() for c in range(self.C)]
        self.list_codes = [codes[lo[c]:lo[c + 1]].copy() for c in range(self.C)]
        self.max_id = int(ids.max()) if ids.size else -1

    @classmethod
    def from_rows(cls, coarse, codebook, ids, cell, codes):
        """rows in any order -> lists ordered by id"""
        ids, cell = np.asarray(ids, np.int32), np.asarray(cell, np.int32)
        order = np.lexsort((ids, cell))
        lo = np.zeros(np.asarray(coarse).shape[0] + 1, np.int32)
        lo[1:] = np.cumsum(np.bincount(cell, minlength=lo.size - 1))
        return cls(coarse, codebook, lo, ids[order], np.asarray(codes, np.int16)[order])

    @property
    def N(self):
        return sum(a.size for a in self.list_ids)

    def list_len(self, c):
        return self.list_ids[c].size

    def append(self, ids, cell=None, codes=None):
        ids = _check_ids(ids, self.max_id)
        if codes is None or cell is None:
            raise Refused("coarse_id and codes are required")
        cell = _check_cells(cell, ids.size, self.C)
        codes = _check_codes(codes, ids.size, self.m, self.K)
        for i in range(ids.size):   # one row at a time: "each row joins the end of its cell's inverted list"
            c = int(cell[i])
            self.list_ids[c] = np.concatenate([self.list_ids[c], ids[i:i + 1]])
            self.list_codes[c] = np.concatenate([self.list_codes[c], codes[i:i + 1]])
        self.max_id = int(ids[-1])

    def update_codebook(self, codebook):
        self.codebook = _check_codebook(self.codebook, codebook)

    def tables(self):
        """(list_off, ids, codes) as freddy_ivf_desc wants them"""
        lo = np.zeros(self.C + 1, np.int32)
        lo[1:] = np.cumsum([a.size for a in self.list_ids])
        return lo, np.concatenate(self.list_ids).astype(np.int32), np.concatenate(self.list_codes).astype(np.int16).reshape(-1, self.m)

    def pin_args(self):
        lo, ids, codes = self.tables()
        return self.coarse, self.codebook, lo, ids, codes

    def oracle_table(self, oracle):
        return oracle.ivf_table(*self.pin_args())


class IVPQModel:
    """codebook_ivpq + coarse multi-index + fine_quantization_ivpq (+ vectors, statistics): rows in id order with their cell."""

    def __init__(self, codebook, coarse, ids, cell, codes, vectors, stats):
        self.codebook = np.ascontiguousarray(codebook, np.float32).copy()
        self.coarse = np.ascontiguousarray(coarse, np.float32).copy()
        self.m, self.K, _ = self.codebook.shape
        self.cells = self.coarse.shape[1] ** 2
        self.ids = np.ascontiguousarray(ids, np.int32).copy()
        self.cell = np.ascontiguousarray(cell, np.int32).copy()
        self.codes = np.ascontiguousarray(codes, np.int16).reshape(self.ids.size, self.m).copy()
        self.vectors = None if vectors is None else np.ascontiguousarray(vectors, np.float32).copy()
        self.stats = np.ascontiguousarray(stats, np.float32).copy()   # (the statistics row is not part of a mutation)

    @property
    def N(self):
        return self.ids.size

    @property
    def ids_affine(self):
        return self.N > 0 and int(self.ids[-1]) - int(self.ids[0]) == self.N - 1

    def append(self, ids, cell=None, codes=None, vectors=None):
        ids = _check_ids(ids, self.ids[-1] if self.N else -1)
        if codes is None or cell is None or (self.vectors is not None and vectors is None):
            raise Refused("coarse_id, codes (and vectors, if pinned) are required")
        cell = _check_cells(cell, ids.size, self.cells)
        codes = _check_codes(codes, ids.size, self.m, self.K)
        self.ids = np.concatenate([self.ids, ids])
        self.cell = np.concatenate([self.cell, cell])
        self.codes = np.concatenate([self.codes, codes])
        if self.vectors is not None:
            self.vectors = np.concatenate([self.vectors, np.ascontiguousarray(vectors, np.float32).reshape(ids.size, -1)])

    def update_codebook(self, codebook):
        self.codebook = _check_codebook(self.codebook, codebook)

    def pin_args(self):
        return self.codebook, self.coarse, self.ids, self.cell, self.codes, self.vectors, self.stats

    def oracle_table(self, oracle):
        return oracle.ivpq_table(*self.pin_args())


class VecModel:
    """google_vecs_norm as raw vectors: rows in id order.  There is no codebook: update_codebook is refused."""

    def __init__(self, ids, vectors):
        self.ids = np.ascontiguousarray(ids, np.int32).copy()
        self.vectors = np.ascontiguousarray(vectors, np.float32).copy()

    @property
    def N(self):
        return self.ids.size

    def append(self, ids, vectors=None):
        ids = _check_ids(ids, self.ids[-1] if self.N else -1)
        if vectors is None:
            raise Refused("vectors are required")
        self.ids = np.concatenate([self.ids, ids])
        self.vectors = np.concatenate([self.vectors, np.ascontiguousarray(vectors, np.float32).reshape(ids.size, -1)])

    def update_codebook(self, codebook):
        raise Refused("a vector handle has no codebook")

    def pin_args(self):
        return self.ids, self.vectors

    def oracle_table(self, oracle):
        """oracle.exact_knn takes the arrays themselves: (vectors, ids)"""
        return self.vectors, self.ids
