"""Plain-Python model of freddy_gpu_update_rows (include/freddy_gpu.h) on the tables behind a pinned handle: the classes of
tests/removal_model.py with an update(...) method beside append and remove.

update(ids, payload...) -> the number of rows that changed.  For every i whose ids[i] is the id of a row, that row's payload
becomes the i-th one given; its id stays, and so do N and an ivf model's max_id.  ids may come in any order; an id no row has is
skipped, but its payload is validated like the others.  A flat row stays where it is; an ivf row whose cell stays keeps its place
in its list, one whose cell changes leaves its list (the others keep their order) and joins the new one.  The model keeps every
list in id order, as a fresh pin requires its lists: the table rebuilt from scratch with the rows replaced.  The handle puts such
a row at the END of its new list instead; the order inside a list never decides a result.

Raises Refused and leaves the model as it was: an id listed twice, a negative id, a payload array the kind needs but did not
get, a cell outside the cells, a code outside [0, K)."""
import numpy as np

import mutation_model as mm
import removal_model as rm
from mutation_model import Refused   # noqa: F401  (the tests catch it through this module)


def _check_update_ids(ids):
    if ids is None:
        raise Refused("ids are required")
    ids = np.asarray(ids).reshape(-1)
    bad = np.nonzero(ids < 0)[0]
    if bad.size:
        raise Refused(f"id {int(ids[bad[0]])} at position {int(bad[0])} is negative")
    order = np.argsort(ids, kind="stable")
    twice = np.nonzero(ids[order][1:] == ids[order][:-1])[0]
    if twice.size:
        j = int(twice[0])
        raise Refused(f"id {int(ids[order][j])} is listed twice, at positions {int(order[j])} and {int(order[j + 1])}")
    return ids.astype(np.int32)


def _rows_of(table_ids, ids):
    """(positions in ids whose id the ascending table_ids has, the rows they name)"""
    r = np.searchsorted(table_ids, ids)
    inside = r < table_ids.size
    hit = np.zeros(ids.size, bool)
    hit[inside] = table_ids[r[inside]] == ids[inside]
    return np.nonzero(hit)[0], r[hit]


class PQModel(rm.PQModel):
    def update(self, ids, codes=None):
        ids = _check_update_ids(ids)
        codes = mm._check_codes(codes, ids.size, self.m, self.K)
        at, rows = _rows_of(self.ids, ids)
        self.codes[rows] = codes[at]
        return int(rows.size)


class IVFModel(rm.IVFModel):
    def update(self, ids, cell=None, codes=None):
        ids = _check_update_ids(ids)
        if codes is None or cell is None:
            raise Refused("coarse_id and codes are required")
        cell = mm._check_cells(cell, ids.size, self.C)
        codes = mm._check_codes(codes, ids.size, self.m, self.K)
        where = {}
        for c in range(self.C):
            for r, i in enumerate(self.list_ids[c].tolist()):
                where[i] = (c, r)
        changed, moved = 0, []
        for i in np.argsort(ids, kind="stable").tolist():
            if int(ids[i]) not in where:
                continue
            changed += 1
            c, r = where[int(ids[i])]
            if c == int(cell[i]):
                self.list_codes[c][r] = codes[i]
            else:
                moved.append((i, c))
        for c in {c for _, c in moved}:   # out of the old lists, the rows that stay in their order
            keep = ~np.isin(self.list_ids[c], ids[[i for i, cc in moved if cc == c]])
            self.list_ids[c], self.list_codes[c] = self.list_ids[c][keep], self.list_codes[c][keep]
        for i, _ in moved:                # into the new ones, at their place in id order
            c = int(cell[i])
            at = int(np.searchsorted(self.list_ids[c], ids[i]))
            self.list_ids[c] = np.insert(self.list_ids[c], at, ids[i])
            self.list_codes[c] = np.insert(self.list_codes[c], at, codes[i], axis=0)
        return changed

    def cell_of(self, ids):
        """the cell of every id (-1: no row has it)"""
        out = np.full(np.asarray(ids).size, -1, np.int32)
        for c in range(self.C):
            out[np.isin(ids, self.list_ids[c])] = c
        return out


class IVPQModel(rm.IVPQModel):
    def update(self, ids, cell=None, codes=None, vectors=None):
        ids = _check_update_ids(ids)
        if codes is None or cell is None or (self.vectors is not None and vectors is None):
            raise Refused("coarse_id, codes (and vectors, if pinned) are required")
        cell = mm._check_cells(cell, ids.size, self.cells)
        codes = mm._check_codes(codes, ids.size, self.m, self.K)
        at, rows = _rows_of(self.ids, ids)
        self.cell[rows], self.codes[rows] = cell[at], codes[at]
        if self.vectors is not None:
            self.vectors[rows] = np.ascontiguousarray(vectors, np.float32).reshape(ids.size, -1)[at]
        return int(rows.size)


class VecModel(rm.VecModel):
    def update(self, ids, vectors=None):
        ids = _check_update_ids(ids)
        if vectors is None:
            raise Refused("vectors are required")
        at, rows = _rows_of(self.ids, ids)
        self.vectors[rows] = np.ascontiguousarray(vectors, np.float32).reshape(ids.size, -1)[at]
        return int(rows.size)
