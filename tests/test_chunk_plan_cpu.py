"""The chunk sizes of the search calls (postgres-word2vec_amd/csrc/chunk_plan.h) on their own: how many queries of a call share one
workspace within option lut_budget_mb, for the IVFADC calls and for the flat PQ table's two paths.

chunk_plan.h is plain C++ (no HIP): compiled here with g++ into a small program with its own main, once as it is and once with
-fsanitize=address,undefined, as test_stage_plan_cpu.py compiles the staging decisions.  The program answers one question per line
of stdin; every answer is compared with the restatement in tests/chunk_inputs.py over a sweep that reaches every regime of the
IVFADC formula (special, special-lut, multi, wide, bigk, long, bucket) and every clamp: n < 1 and n > 2^20 of the IVFADC and the
generic PQ sizes, the 256 MiB / (4 C) bucket cap, the cell-grouped PQ scan's floor of 16 and ceiling of 2^16.

The bucket cap binds only with tens of thousands of cells (256 MiB / (4 C) queries against budget / 32 KiB): no GPU test pins such
a table, so that regime is covered here alone.  Every other regime is reached by a case of tests/test_gpu_chunks.py;
test_gpu_cases_reach_their_regimes asserts, per GPU case, the regime, the budget that dials its chunk size and the chunks it gets."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chunk_inputs as ci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
#include "chunk_plan.h"
using namespace freddy;
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char what;
    in >> what;
    if (what == 'I') {          // I mb m K W k upi special C max_list_blocks
      long long mb; int m, K, W, k, upi, special, C, mlb;
      in >> mb >> m >> K >> W >> k >> upi >> special >> C >> mlb;
      printf("%d\n", max_queries_per_chunk(mb, m, K, W, k, upi, special != 0, C, mlb));
    } else if (what == 'F') {   // F mb n_blocks
      long long mb, nb;
      in >> mb >> nb;
      printf("%d\n", pq_fused_queries_per_chunk(mb, nb));
    } else if (what == 'G') {   // G mb m K n_blocks k
      long long mb, nb; int m, K, k;
      in >> mb >> m >> K >> nb >> k;
      printf("%d\n", pq_queries_per_chunk(mb, m, K, nb, k));
    }
  }
  return 0;
}
"""

# (name, arguments of ivf_per, the regime names it must carry, the size if it is a clamp's)
EDGES = [
    ("n < 1: 512 probes of a K = 1024 table in 1 MB", (1, 12, 1024, 512, 5, 1, 1, 64, 64), {"special-lut"}, 1),
    ("n > 2^20: one probe of a tiny table under 2^16 MB", (1 << 16, 2, 4, 1, 1, 40, 0, 8, 2560), {"long"}, 1 << 20),
    ("bucket cap: 70 000 cells under the default budget", (8192, 12, 256, 1, 5, 1, 1, 70000, 64), {"special", "bucket"}, (256 << 20) // (4 * 70000)),
    ("bucket cap, multi shape: 20 000 cells", (8192, 5, 256, 1, 5, 1, 0, 20000, 64), {"multi", "bucket"}, (256 << 20) // (4 * 20000)),
    ("no cap without survivor bytes: 70 000 cells, nine units", (8192, 12, 256, 1, 5, 9, 1, 70000, 576), {"long"}, (8192 << 20) // (12 * 1024)),
    ("nprobe 10, lists of two units, 8 GiB: the workload's 12 800 queries are one chunk", (8192, 12, 1024, 10, 10, 2, 1, 1000, 128), {"special"}, (8192 << 20) // (20 * ci.SURV_UNIT)),
    ("eight units still have survivor regions", (64, 12, 256, 2, 5, 8, 1, 64, 512), {"special"}, 128),
    ("thirty-two units of a multi shape", (64, 5, 256, 2, 5, 32, 0, 64, 2048), {"multi"}, (64 << 20) // (2 * 5 * 1024 + 64 * ci.SURV_UNIT)),
    ("thirty-three: none", (64, 5, 256, 2, 5, 33, 0, 64, 2112), {"long"}, (64 << 20) // (2 * 5 * 1024)),
    ("C = 0 does not divide by zero", (8, 12, 256, 1, 5, 1, 1, 0, 1), {"special"}, 256),
]


def _questions():
    rng = np.random.default_rng(21)
    qs = [("I",) + e[1] for e in EDGES]
    for _ in range(3000):
        special = int(rng.integers(0, 2))
        m, K = (12, int(rng.choice([16, 64, 256, 1024]))) if special else (int(rng.choice([2, 5, 8, 30])), int(rng.choice([4, 16, 32, 256, 512])))
        mlb = int(rng.choice([0, 1, 63, 64, 65, 256, 257, 512, 513, 2048, 2049, 5000]))
        qs.append(("I", int(rng.choice([1, 2, 3, 33, 48, 1000, 8192, 1 << 16, 1 << 20])), m, K, int(rng.choice([1, 2, 4, 10, 32, 512])),
                   int(rng.choice([1, 5, 32, 33, 40, 512, 513, 600, 1025, 4096])), ci.units_per_item(mlb), special,
                   int(rng.choice([0, 1, 32, 64, 1000, 20000, 70000, 1 << 22])), mlb))
    for mb in (1, 2, 5, 6, 100, 8192, 1 << 16, 1 << 22):
        for nb in (0, 1, 63, 64, 65, 79, 625, 1094, 1 << 16, 1 << 20, 1 << 26):
            qs.append(("F", mb, nb))
            for k in (1, 5, 32, 33, 512, 513, 600, 1025, 4096):
                qs.append(("G", mb, 12, 256, nb, k))
    qs += [("G", 1, 30, 4096, 1 << 20, 4096), ("G", 1 << 22, 1, 2, 0, 1), ("G", 3, 12, 1024, 0, 5)]
    return qs


def _answer(q):
    return str({"I": ci.ivf_per, "F": ci.pq_fused_per, "G": ci.pq_per}[q[0]](*q[1:]))


def _build(tmp, name, extra):
    src = tmp / "chunk_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)] + extra, check=True)
    return exe


def _check(exe):
    qs = _questions()
    run = subprocess.run([str(exe)], input="".join(" ".join(map(str, q)) + "\n" for q in qs), capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-4000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(qs)
    for q, line in zip(qs, lines):
        assert line.strip() == _answer(q), (q, line)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ not on PATH"
    return tmp_path_factory.mktemp("chunk_plan")


def test_edges_say_what_they_mean():
    for what, args, regime, size in EDGES:
        assert ci.ivf_regime(*args) == regime, (what, ci.ivf_regime(*args))
        assert ci.ivf_per(*args) == size, (what, ci.ivf_per(*args))


def test_sweep_reaches_every_regime_and_clamp():
    seen, sizes = set(), set()
    for q in _questions():
        if q[0] == "I":
            seen |= ci.ivf_regime(*q[1:])
            sizes.add(ci.ivf_per(*q[1:]))
    assert seen == {"special", "special-lut", "multi", "wide", "bigk", "long", "bucket"}
    assert {1, 1 << 20} <= sizes
    fused = {ci.pq_fused_per(*q[1:]) for q in _questions() if q[0] == "F"}
    assert {16, 1 << 16} <= fused and any(16 < n < (1 << 16) for n in fused)
    assert (256 << 20) // (4 * ci.cdiv(1 << 26, 64)) in fused, "the bucket cap of the pseudo-lists"
    assert ci.pq_fused_per(1, 0) == ci.pq_fused_per(1, 1) == 32, "no row block counts as one pseudo-list: nothing divides by zero"
    generic = {ci.pq_per(*q[1:]) for q in _questions() if q[0] == "G"}
    assert {1, 1 << 20} <= generic


def test_a_300d_table_costs_32_kib_per_probe():
    """K = 256, lists of at most 4096 rows, C >= 32: 32 KiB x W per query, so W = 32 makes the chunk lut_budget_mb queries"""
    for mb in (1, 2, 31, 33, 64, 65, 200):
        assert ci.ivf_per(mb, *ci.ivf_args("K256", 32, 5)) == mb
        assert ci.ivf_per(mb, *ci.ivf_args("K256", 1, 5)) == 32 * mb


def _ivf_cases():
    return ci.DEV_MATRIX + ci.DEV_REGIMES + [ci.DEV_MIDDLE] + ci.HOST_CALLS + [ci.STRAGGLERS, ci.LAYERS_IVF]


def test_gpu_cases_reach_their_regimes():
    """per case of tests/test_gpu_chunks.py: the budget that dials its chunk size (the same at both ends of the table's bound on its
    longest list), the regime, at least three chunks, and the tail the case is about"""
    reached = set()
    for c in _ivf_cases():
        lo, hi = ci.IVF_TABLES[c["table"]]["max_rows"]
        mb = ci.ivf_budget(c)
        assert mb is not None and mb == ci.ivf_budget(c, lo), c["id"]
        args = ci.ivf_args(c["table"], c["W"], c["k"])
        assert ci.ivf_per(mb, *args) == c["per"] and ci.ivf_regime(mb, *args) == c["regime"], (c["id"], ci.ivf_regime(mb, *args))
        assert ci.ivf_per(ci.DEFAULT_MB, *args) >= 300, c["id"]     # the default budget does not cut the call
        assert len(ci.cuts(c["Q"], c["per"])) >= 3, c["id"]
        reached |= c["regime"]
    assert reached == {"special", "special-lut", "multi", "wide", "bigk", "long"}   # (bucket: the module docstring)
    for c in ci.DEV_MATRIX:
        tail = ci.cuts(c["Q"], c["per"])[-1][1]
        assert len(ci.cuts(c["Q"], c["per"])) == (4 if c["Q"] % 3 else 3) and tail == (1 if c["Q"] % 3 else c["per"]), c["id"]
        # fused = -1: a one-query chunk is below the automatic threshold, a full chunk of 31 or more above it
        assert (1 * c["W"] < ci.AUTO_ITEMS) and ((c["per"] * c["W"] >= ci.AUTO_ITEMS) == (c["per"] >= 31))
    # a sub-batch never holds more queries than a chunk, so its stragglers are re-searched as one chunk (chunk_inputs.STRAGGLERS)
    subs = ci.sub_batches(ci.STRAGGLERS["Q"], ci.STRAGGLERS["per"])
    assert [n for _, n in subs] == [29, 29, 27] and all(len(ci.cuts(n, ci.STRAGGLERS["per"])) == 1 for _, n in subs)
    assert [n for _, n in ci.sub_batches(9, 1)] == [1] * 9 and [n for _, n in ci.sub_batches(100, 33)] == [25] * 4
    mid = ci.cuts(ci.DEV_MIDDLE["Q"], ci.DEV_MIDDLE["per"])
    assert [n for _, n in mid] == [96, 96, 96, 12]


def test_gpu_pq_cases_get_their_chunks():
    for c in ci.PQ_CALLS + [ci.LAYERS_PQ]:
        nb = ci.blocks_of(c["N"])
        mb = ci.pq_budget(c, nb)
        assert mb is not None, c["id"]
        sizes = [n for _, n in ci.cuts(c["Q"], c["per"])]
        assert len(sizes) >= 3, c["id"]
        assert (ci.pq_fused_per(ci.DEFAULT_MB, nb) if c["fused"] else ci.pq_per(ci.DEFAULT_MB, ci.PQ_M, ci.PQ_K, nb, c["k"])) >= c["Q"], c["id"]
    by_id = {c["id"]: [n for _, n in ci.cuts(c["Q"], c["per"])] for c in ci.PQ_CALLS}
    assert by_id["fused-16-Q33"] == [16, 16, 1] and by_id["fused-16-Q48"] == [16, 16, 16] and by_id["fused-19-Q58"] == [19, 19, 19, 1]
    assert by_id["fused-16-Q130"][-1] == 2 and by_id["generic-k32-Q121"] == [60, 60, 1] and by_id["generic-k600-Q55"] == [18, 18, 18, 1]
    assert by_id["generic-k5-N4097-Q169"] == [84, 84, 1] and by_id["generic-k600-N4097-Q47"] == [23, 23, 1]
    # a subset's chunks follow ITS row blocks: the table's 625 blocks would cut the same call into another number of chunks
    sub_nb, table_nb = ci.blocks_of(ci.PQ_SUBSET_ROWS), ci.blocks_of(40000)
    for c in ci.PQ_SUBSETS:
        mb = ci.pq_budget(c, sub_nb)
        assert mb is not None, c["id"]
        own = ci.pq_fused_per(mb, sub_nb) if c["fused"] else ci.pq_per(mb, ci.PQ_M, ci.PQ_K, sub_nb, c["k"])
        other = ci.pq_fused_per(mb, table_nb) if c["fused"] else ci.pq_per(mb, ci.PQ_M, ci.PQ_K, table_nb, c["k"])
        assert own == c["per"] and len(ci.cuts(c["Q"], own)) == 3 and len(ci.cuts(c["Q"], other)) not in (1, 3), c["id"]


def test_program_equals_the_restatement(tmp):
    _check(_build(tmp, "chunk", []))


def test_program_under_the_sanitizers(tmp):
    """the same program built with AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded,
    nothing sanitised is loaded into Python): the same answers, and no report"""
    _check(_build(tmp, "chunk_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"]))
