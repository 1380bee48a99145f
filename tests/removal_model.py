"""Plain-Python model of freddy_gpu_remove_rows (include/freddy_gpu.h) on the tables behind a pinned handle: the classes of
tests/mutation_model.py with a remove(ids) method.

remove(ids) -> the number of rows that left.  ids may come in any order, an id listed twice counts once, an id no row has is
skipped; the rows that stay keep their order (inside its list, for an ivf row); an ivf model's max_id becomes the largest id
that is left (-1: none), so that a later append may start above it, as on a fresh pin.  A negative id raises Refused and
leaves the model as it was."""
import numpy as np

import mutation_model as mm
from mutation_model import Refused   # noqa: F401  (the tests catch it through this module)


def _check_remove(ids):
    if ids is None:
        raise Refused("ids are required")
    ids = np.asarray(ids).reshape(-1)
    bad = np.nonzero(ids < 0)[0]
    if bad.size:
        raise Refused(f"id {int(ids[bad[0]])} at position {int(bad[0])} is negative")
    return ids.astype(np.int32)


class PQModel(mm.PQModel):
    def remove(self, ids):
        keep = ~np.isin(self.ids, _check_remove(ids))
        gone = int(self.N - keep.sum())
        self.ids, self.codes = self.ids[keep], self.codes[keep]
        return gone


class IVFModel(mm.IVFModel):
    def remove(self, ids):
        ids = _check_remove(ids)
        gone = 0
        for c in range(self.C):
            keep = ~np.isin(self.list_ids[c], ids)
            gone += int(keep.size - keep.sum())
            self.list_ids[c], self.list_codes[c] = self.list_ids[c][keep], self.list_codes[c][keep]
        self.max_id = max((int(a.max()) for a in self.list_ids if a.size), default=-1)
        return gone


class IVPQModel(mm.IVPQModel):
    def remove(self, ids):
        keep = ~np.isin(self.ids, _check_remove(ids))
        gone = int(self.N - keep.sum())
        self.ids, self.cell, self.codes = self.ids[keep], self.cell[keep], self.codes[keep]
        if self.vectors is not None:
            self.vectors = self.vectors[keep]
        return gone


class VecModel(mm.VecModel):
    def remove(self, ids):
        keep = ~np.isin(self.ids, _check_remove(ids))
        gone = int(self.N - keep.sum())
        self.ids, self.vectors = self.ids[keep], self.vectors[keep]
        return gone
