"""freddy_gpu_encode_rows / freddy_gpu_last_encode_stats exist in every layer -- exported by libfreddy_gpu.so, declared in
include/freddy_gpu.h with ABI version 4, listed and bound in freddy_amd/gpu.py -- and every refusal that needs no pinned handle is
reported before a device is touched (the ones that compare with a handle's d / N / state: tests/test_gpu_encode_rows.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("freddy_gpu_encode_rows", "freddy_gpu_last_encode_stats")
E_ARG, E_LIMIT = -1, -5


def test_declared_exported_and_bound():
    from freddy_amd import gpu
    lib = gpu.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "freddy_gpu.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, hdr), f"{n} is not declared"
        assert hasattr(lib, n) and getattr(lib, n).argtypes, f"{n} is not exported / bound"
        assert n in gpu.EXPORTS, n
    assert lib.freddy_gpu_abi_version() == 4 and "#define FREDDY_GPU_ABI_VERSION 4" in hdr and gpu.ABI_VERSION == 4
    assert callable(gpu.VectorIndex.encode_rows) and callable(gpu.VectorIndex.last_encode_stats)
    assert '"encode_refine_all"' in open(os.path.join(ROOT, "include", "freddy_gpu.h")).read()


# (what is wrong, the code, a word of the message): d, m, K, C, which pointers are NULL
REFUSALS = [
    ("desc", E_ARG, "NULL"), ("codebook", E_ARG, "NULL"), ("out_codes", E_ARG, "NULL"),
    (dict(d=25, m=4), E_ARG, "bad shape"), (dict(K=32768), E_LIMIT, "int16"),
    (dict(C=3, coarse=False), E_ARG, "together"), (dict(C=0, coarse=True), E_ARG, "together"),
    (dict(C=3, out_cell=False), E_ARG, "out_cell"), ("handle", E_ARG, "NULL index"),
]


@pytest.mark.parametrize("what,code,word", REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_refusals_without_a_device(what, code, word):
    from freddy_amd import gpu
    lib = gpu.load()
    o = dict(d=24, m=6, K=31, C=0, coarse=None, out_cell=True)
    if isinstance(what, dict):
        o.update(what)
    if o["coarse"] is None:
        o["coarse"] = o["C"] > 0
    cb, co = np.zeros(8, np.float32), np.zeros(8, np.float32)   # (never read: every case is refused first)
    cell, codes = np.full(4, 7, np.int32), np.full(4, 7, np.int16)
    desc = gpu.EncodeDesc(o["d"], o["m"], o["K"], None if what == "codebook" else gpu._p(cb), o["C"], gpu._p(co) if o["coarse"] else None)
    rc = lib.freddy_gpu_encode_rows(None, None if what == "desc" else C.byref(desc), 0, 4, gpu._p(cell) if o["out_cell"] else None,
                                    None if what == "out_codes" else gpu._p(codes))
    assert rc == code, (rc, lib.freddy_gpu_last_error())
    assert word.encode() in lib.freddy_gpu_last_error()
    assert (cell == 7).all() and (codes == 7).all()          # a refused call writes nothing
    out = (C.c_int64 * 5)()
    assert lib.freddy_gpu_last_encode_stats(None, out) == E_ARG
