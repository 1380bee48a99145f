"""The tokenize case list (tests/tokenize_inputs.py) can tell wrong implementations apart, and the model (tests/tokenize_model.py)
computes the reference's loop.  No GPU.
For every shape the inputs themselves show, in bits, that
  * the TABLE_ORDER and the POSITIONAL centroid of some text differ (duplicates and unknown ids count);
  * summing a duplicate-free text in the given order differs from summing it in table order;
  * x / n differs from x * (1 / n) for some element;
  * dividing the finished sum by n differs from the reference's loop;
  * a pairwise (tree) summation differs from the sequential one at some length >= 64.
The model's centroid is compared with tests/tokenize_centroid_check.c, the loop in C: built plain, and built with ASan + UBSan
(their runtimes linked into the program) and run as it is."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tokenize_inputs as ti
import tokenize_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
U = np.uint32


def _differ(a, b):
    return not np.array_equal(np.asarray(a, np.float32).view(U), np.asarray(b, np.float32).view(U))


def _cases(d):
    ids, v = ti.table(d)
    return ids, v, ti.texts(ids)


def test_the_case_list_has_every_length_and_kind():
    ids, v, texts = _cases(300)
    assert ids.size == ti.N_ROWS and np.all(np.diff(ids) > 0) and np.any(np.diff(ids) > 1)
    assert sorted({len(t) for _, t in texts}) == sorted(ti.LENGTHS) and max(ti.LENGTHS) == tm.MAX_LEN
    names = [n for n, _ in texts]
    for L in ti.LENGTHS[1:]:
        for kind in ("unsorted", "duplicates", "mixed", "unknown"):
            assert f"len{L}_{kind}" in names
    for name, t in texts:
        rows = tm.rows_of(ids, t)
        if name.endswith("_unknown"):
            assert np.all(rows < 0), name
        if name.endswith("_mixed") and len(t) >= 2:
            assert np.any(rows < 0) and np.any(rows >= 0), name
        if name.endswith("_duplicates") and len(t) >= 2:
            assert len(np.unique(t)) < len(t), name
        if name.endswith("_unsorted") and 2 <= len(t) <= ids.size:
            assert len(np.unique(t)) == len(t) and np.any(np.diff(rows) < 0), name
    assert np.any(np.signbit(v) & (v == 0)) and np.any(~np.signbit(v) & (v == 0))
    mag = np.abs(v[v != 0])
    assert mag.min() < 2.0 ** -30 and mag.max() > 2.0 ** 30


@pytest.mark.parametrize("d", ti.SHAPES)
def test_the_inputs_tell_wrong_implementations_apart(d):
    ids, v, texts = _cases(d)
    rule_differs = order_differs = recip_differs = late_division_differs = tree_differs = False
    for name, t in texts:
        pos, tab = tm.row_list(ids, t, tm.POSITIONAL), tm.row_list(ids, t, tm.TABLE_ORDER)
        if len(pos) == 0:
            continue
        c_pos, c_tab = tm.centroid(v, pos), tm.centroid(v, tab)
        if name.endswith(("_duplicates", "_mixed")) and _differ(c_pos, c_tab):
            rule_differs = True
        if name.endswith("_unsorted") and len(pos) == len(tab) and _differ(c_pos, c_tab):
            order_differs = True
        n = np.float32(len(tab))
        rows = v[tab]
        if _differ(rows / n, rows * (np.float32(1) / n)):
            recip_differs = True
        s = np.zeros(d, np.float32)
        for r in rows:
            s = s + r
        if _differ(s / n, c_tab):
            late_division_differs = True
        if len(tab) >= 64:
            terms = [r / n for r in rows]
            while len(terms) > 1:
                terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            if _differ(terms[0], c_tab):
                tree_differs = True
    assert rule_differs and order_differs and recip_differs and late_division_differs and tree_differs, \
        (rule_differs, order_differs, recip_differs, late_division_differs, tree_differs)


@pytest.mark.parametrize("kind", ["plain", "asan_ubsan"])
def test_the_model_centroid_equals_the_loop_in_c(kind, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = str(tmp_path / ("tokenize_centroid_check_" + kind))
    flags = ["-O2"]
    if kind == "asan_ubsan":
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                 "-static-libasan", "-static-libubsan"]
    subprocess.check_call([cc] + flags + ["-std=c11", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe,
                                          os.path.join(HERE, "tokenize_centroid_check.c")])
    for d in ti.SHAPES:
        ids, v, texts = _cases(d)
        lists = [tm.row_list(ids, t, rule) for _, t in texts for rule in (tm.TABLE_ORDER, tm.POSITIONAL)]
        src, dst = str(tmp_path / f"in_{d}.bin"), str(tmp_path / f"out_{d}.bin")
        with open(src, "wb") as f:
            f.write(np.array([len(lists), d], np.int32).tobytes())
            for rows in lists:
                f.write(np.array([len(rows)], np.int32).tobytes())
                f.write(np.ascontiguousarray(v[rows], np.float32).tobytes())
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        got = np.fromfile(dst, np.float32).reshape(len(lists), d)
        for i, rows in enumerate(lists):
            assert not _differ(got[i], tm.centroid(v, rows)), (d, i, len(rows))
