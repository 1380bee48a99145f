"""The block plan (postgres-word2vec_amd/csrc/block_plan.h) on its own: list lengths -> list_off, blk_off, blk_cell,
max_list_blocks, n_blocks -- what pack_lists, the append and the removal of the pinned pq / ivf layouts all derive from one function.

block_plan.h is plain C++ (no HIP): compiled here with g++ into a small program with its own main, once as it is and once with
-fsanitize=address,undefined, as test_alloc_hook_cpu.py compiles the allocation seam.  Both programs read the same cases from
stdin and print the plan; every figure is compared with a numpy restatement.  The cases: an empty table (every length 0: no
block, one block allocated), lengths from {0, 1, 63, 64, 65, 128, 129} (around one and two blocks), a single list (the flat
table), and totals one row under, at, and one row over the 32-bit limit of INT32_MAX - 64 rows, from three huge lengths: the last
is refused, as are a single list over the limit and a negative length.  For the huge totals blk_cell (one int per block, 134 MB:
the only large array, and the plan's own) is not printed; the program compares it with blk_off run by run and prints the number
of blocks that disagree."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")
LIMIT = 2 ** 31 - 1 - 64
PRINT_UP_TO = 100000          # blocks: beyond that blk_cell is checked inside the program only
OK, NEGATIVE, TOO_MANY = 0, 1, 2

PROGRAM = r"""
#include <stdio.h>
#include <sstream>
#include <string>
#include <iostream>
#include "block_plan.h"
using namespace freddy;
// stdin: one case per line, the lists' lengths.  stdout per case:
//   rc bad | n_blocks allocated max_list_blocks disagreeing | list_off ... | blk_off ... | blk_cell ... (small plans only)
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<long long> len;
    for (long long v; in >> v;) len.push_back(v);
    BlockPlan p;
    int bad = -1;
    const int rc = plan_blocks((int)len.size(), [&](int c) { return (int64_t)len[(size_t)c]; }, p, &bad);
    printf("%d %d |", rc, bad);
    if (rc == PLAN_OK) {
      long long disagree = 0;
      for (size_t c = 0; c < len.size(); ++c)
        for (int32_t b = p.blk_off[c]; b < p.blk_off[c + 1]; ++b) disagree += p.blk_cell[(size_t)b] != (int32_t)c;
      printf(" %lld %zu %d %lld |", (long long)p.n_blocks, p.blk_cell.size(), p.max_list_blocks, disagree);
      for (int32_t v : p.list_off) printf(" %d", v);
      printf(" |");
      for (int32_t v : p.blk_off) printf(" %d", v);
      printf(" |");
      if (p.blk_cell.size() <= PRINT_UP_TO)
        for (int32_t v : p.blk_cell) printf(" %d", v);
    }
    printf("\n");
  }
  return 0;
}
"""


def _cases():
    rng = np.random.default_rng(64)
    steps = [0, 1, 63, 64, 65, 128, 129]
    cases = [[0], [0] * 5, steps, steps[::-1], [129], [64], [1000], [4097]]
    cases += [[v] for v in steps]
    cases += [list(rng.choice(steps, size=n)) for n in (2, 7, 40, 257)]
    a, b = 2 ** 30, 2 ** 29 - 1
    cases += [[a, b, LIMIT - 1 - a - b], [a, b, LIMIT - a - b], [a, b, LIMIT + 1 - a - b], [0, LIMIT + 1], [2 ** 40], [5, -1, 5]]
    return [[int(v) for v in c] for c in cases]


def _model(lens):
    """the plan restated: (rc, bad) and, for an accepted plan, its figures (blk_cell None where it is too long to print)"""
    lens = np.asarray(lens, np.int64)
    total = 0
    for c, n in enumerate(lens):
        if n < 0:
            return (NEGATIVE, c), None
        total += int(n)
        if total > LIMIT:
            return (TOO_MANY, c), None
    nb = (lens + 63) // 64
    list_off = np.concatenate([[0], np.cumsum(lens)])
    blk_off = np.concatenate([[0], np.cumsum(nb)])
    n_blocks = int(blk_off[-1])
    allocated = max(n_blocks, 1)
    blk_cell = None
    if allocated <= PRINT_UP_TO:
        blk_cell = np.repeat(np.arange(len(lens)), nb) if n_blocks else np.zeros(1, np.int64)
    return (OK, len(lens) - 1), dict(n_blocks=n_blocks, allocated=allocated, max_list_blocks=int(nb.max()), list_off=list_off, blk_off=blk_off, blk_cell=blk_cell)


def _build(tmp, name, extra):
    src = tmp / "plan_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-DPRINT_UP_TO=%d" % PRINT_UP_TO, "-I" + CSRC, str(src), "-o", str(exe)] + extra, check=True)
    return exe


def _check(exe):
    cases = _cases()
    run = subprocess.run([str(exe)], input="".join(" ".join(map(str, c)) + "\n" for c in cases), capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-4000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    accepted = refused = 0
    for lens, line in zip(cases, lines):
        parts = [np.array(p.split(), np.int64) for p in line.split("|")]
        (rc, bad), exp = _model(lens)
        assert parts[0][0] == rc, (lens[:8], line[:200])
        if rc != OK:
            assert parts[0][1] == bad and len(parts) == 2 and parts[1].size == 0, (lens[:8], line[:200])
            refused += 1
            continue
        accepted += 1
        n_blocks, allocated, max_list_blocks, disagree = parts[1]
        assert (n_blocks, allocated, max_list_blocks, disagree) == (exp["n_blocks"], exp["allocated"], exp["max_list_blocks"], 0), (lens[:8], line[:200])
        assert np.array_equal(parts[2], exp["list_off"]) and np.array_equal(parts[3], exp["blk_off"]), (lens[:8], line[:200])
        if exp["blk_cell"] is not None:
            assert np.array_equal(parts[4], exp["blk_cell"]), (lens[:8], line[:200])
        else:
            assert parts[4].size == 0
    assert accepted == len(cases) - 4 and refused == 4


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not on PATH")
    return tmp_path_factory.mktemp("block_plan")


def test_model_covers_the_cases():
    """the cases hold what they are meant to: an empty table, a list of every length around the block size, the flat table, and
    totals on both sides of the limit"""
    cases = _cases()
    plans = [_model(c) for c in cases]
    assert any(p[1] and p[1]["n_blocks"] == 0 and p[1]["allocated"] == 1 and len(c) > 1 for c, p in zip(cases, plans))
    assert {v for c in cases for v in c} >= {0, 1, 63, 64, 65, 128, 129}
    assert any(len(c) == 1 and p[0][0] == OK and p[1]["n_blocks"] > 1 for c, p in zip(cases, plans))
    totals = {sum(c): p[0][0] for c, p in zip(cases, plans) if len(c) == 3 and min(c) > 2 ** 20}
    assert totals == {LIMIT - 1: OK, LIMIT: OK, LIMIT + 1: TOO_MANY}


def test_plan_equals_the_numpy_restatement(tmp):
    _check(_build(tmp, "plan", []))


def test_plan_under_the_sanitizers(tmp):
    """the same program built with AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded,
    nothing sanitised is loaded into Python): the same figures, and no report"""
    exe = _build(tmp, "plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"])
    _check(exe)
