"""The similarities by row id (include/freddy_gpu.h: freddy_gpu_similarity_pairs / _matrix / _join) are declared, exported and bound,
and report their argument errors without a GPU -- scalars and NULL buffers before the handle is looked at."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["freddy_gpu_similarity_pairs", "freddy_gpu_similarity_matrix", "freddy_gpu_similarity_join"]
E_ARG, E_LIMIT = -1, -5


def _lib():
    import __graft_entry__ as g
    g.build()
    from freddy_amd import gpu
    return gpu, gpu.load()


def test_the_three_symbols_are_declared_exported_and_bound():
    gpu, lib = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "freddy_gpu.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, hdr), f"{n} is not declared"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in gpu.EXPORTS and getattr(lib, n).argtypes, n
    assert lib.freddy_gpu_abi_version() == 4 and "#define FREDDY_GPU_ABI_VERSION 4" in hdr
    for m in ("similarity_pairs", "similarity_matrix", "similarity_join"):
        assert callable(getattr(gpu.VectorIndex, m))


def test_argument_errors_are_reported_without_a_gpu():
    gpu, lib = _lib()
    ids = (C.c_int32 * 8)()
    fl = (C.c_float * 64)()
    kn = (C.c_uint8 * 8)()
    total = C.c_int64(7)
    err = lambda: lib.freddy_gpu_last_error().decode()
    thr = C.c_float(0.5)
    fake = C.c_void_p(8)          # a handle that is never looked at: every call below is refused before that

    # pairs
    assert lib.freddy_gpu_similarity_pairs(None, ids, ids, 1, fl, kn) == E_ARG and "NULL index" in err()
    assert lib.freddy_gpu_similarity_pairs(fake, ids, ids, -1, fl, kn) == E_ARG and "n=-1" in err()
    for args in ((None, ids, fl, kn), (ids, None, fl, kn), (ids, ids, None, kn), (ids, ids, fl, None)):
        assert lib.freddy_gpu_similarity_pairs(fake, args[0], args[1], 1, args[2], args[3]) == E_ARG and "NULL buffer" in err()

    # matrix
    m = lib.freddy_gpu_similarity_matrix
    assert m(None, ids, None, 1, ids, 1, fl, kn, kn) == E_ARG and "NULL index" in err()
    assert m(fake, ids, None, -1, ids, 1, fl, kn, kn) == E_ARG and "na=-1" in err()
    assert m(fake, ids, None, 1, ids, -2, fl, kn, kn) == E_ARG and "nb=-2" in err()
    assert m(fake, ids, fl, 1, ids, 1, fl, kn, kn) == E_ARG and "exactly one" in err()
    assert m(fake, None, None, 1, ids, 1, fl, kn, kn) == E_ARG and "exactly one" in err()
    assert m(fake, ids, None, 1, None, 1, fl, kn, kn) == E_ARG and "NULL buffer" in err()
    for args in ((None, kn, kn), (fl, None, kn), (fl, kn, None)):
        assert m(fake, ids, None, 1, ids, 1, *args) == E_ARG and "NULL buffer" in err()
    assert m(fake, ids, None, 1, ids, (1 << 22) + 1, fl, kn, kn) == E_LIMIT and str((1 << 22) + 1) in err()
    assert m(None, ids, None, 1, ids, 1 << 40, fl, kn, kn) == E_LIMIT and str(1 << 40) in err()      # the scalars before the handle

    # join: a refused call leaves n_pairs as it was
    j = lib.freddy_gpu_similarity_join
    refused = [
        (j(None, ids, None, 1, ids, 1, thr, 4, ids, ids, fl, C.byref(total)), E_ARG, "NULL index"),
        (j(fake, ids, None, -1, ids, 1, thr, 4, ids, ids, fl, C.byref(total)), E_ARG, "na=-1"),
        (j(fake, ids, fl, 1, ids, 1, thr, 4, ids, ids, fl, C.byref(total)), E_ARG, "exactly one"),
        (j(fake, None, None, 1, ids, 1, thr, 4, ids, ids, fl, C.byref(total)), E_ARG, "exactly one"),
        (j(fake, ids, None, 1, ids, (1 << 22) + 1, thr, 4, ids, ids, fl, C.byref(total)), E_LIMIT, str((1 << 22) + 1)),
        (j(fake, ids, None, 1, ids, 1, thr, -1, ids, ids, fl, C.byref(total)), E_ARG, "max_pairs=-1"),
        (j(fake, ids, None, 1, ids, 1, thr, 4, None, ids, fl, C.byref(total)), E_ARG, "NULL buffer"),
        (j(fake, ids, None, 1, ids, 1, thr, 4, ids, None, fl, C.byref(total)), E_ARG, "NULL buffer"),
        (j(fake, ids, None, 1, ids, 1, thr, 4, ids, ids, None, C.byref(total)), E_ARG, "NULL buffer"),
        (j(fake, ids, None, 1, ids, 1, thr, 0, None, None, None, None), E_ARG, "NULL n_pairs"),
    ]
    # (the message of each call is gone with the next: the codes here, the messages one by one below)
    for rc, code, _ in refused:
        assert rc == code
    assert total.value == 7
    assert j(fake, ids, None, 1, ids, 1, thr, -1, ids, ids, fl, C.byref(total)) == E_ARG and "max_pairs=-1" in err()
    assert j(None, ids, None, 1, ids, 1, thr, 0, None, None, None, C.byref(total)) == E_ARG and "NULL index" in err()   # a count call needs no outputs
    assert total.value == 7
