"""The staging decisions of the host-buffer calls (postgres-word2vec_amd/csrc/stage_plan.h) on their own: how a call is cut into
sub-batches and lanes, how a sub-batch's queries reach the device, the pieces a chunk's queries cross in, the 16-byte words of a
piece and the layout of the pinned result block.

stage_plan.h is plain C++ (no HIP): compiled here with g++ into a small program with its own main, once as it is and once with
-fsanitize=address,undefined, as test_block_plan_cpu.py compiles the block plan.  The program answers one question per line of
stdin; every answer is compared with a restatement in Python, and the properties the pipeline relies on are asserted on top:
  pieces   Q = 512, 545, 1024, 1999 in four pieces: whole 32-query tiles, every query in exactly one piece, and for d = 300 every
           piece starts on a 16-byte word and the pieces' word ranges tile the sub-batch's block
  source   the ways a sub-batch's queries reach the device, over the cases tests/test_gpu_pipeline.py runs on the GPU: a handful
           read in place from pageable staging or from the caller's pinned buffer, pinned but off a 16-byte word (d = 35: rows of
           140 bytes) -> staged, one row of a device table in place, larger sub-batches by copy kernel or gather
  cuts     sub-batches, lanes and slots of a call, the GPU tests' calls among them"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
#include "stage_plan.h"
using namespace freddy;
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char what;
    in >> what;
    if (what == 'P') {          // P Q pieces -> q_lo q_n per piece
      int Q, pieces;
      in >> Q >> pieces;
      const int rc = for_pieces(Q, pieces, [](int q_lo, int q_n) { printf("%d %d ", q_lo, q_n); return 0; });
      printf("| %d\n", rc);
    } else if (what == 'W') {   // W row q_lo q_hi n stage -> b_lo b_hi w0 w1 cuts per16 aligned | the cuts' word ranges
      size_t row; int q_lo, q_hi, n, stage;
      in >> row >> q_lo >> q_hi >> n >> stage;
      const PieceWords w = piece_words(row, q_lo, q_hi, n, stage != 0);
      printf("%zu %zu %zu %zu %d %zu %d |", w.b_lo, w.b_hi, w.w0, w.w1, w.cuts, w.per16, (int)w.aligned());
      for (int ci = 0; ci < w.cuts && w.cut_lo(ci) < w.cut_hi(ci); ++ci) printf(" %zu %zu", w.cut_lo(ci), w.cut_hi(ci));
      printf("\n");
    } else if (what == 'S') {   // S host pinned row n -> in_place stage
      int host, n; unsigned long long pinned; size_t row;
      in >> host >> pinned >> row >> n;
      const QuerySource s = query_source(host != 0, (uintptr_t)pinned, row, n);
      printf("%d %d\n", (int)s.in_place, (int)s.stage);
    } else if (what == 'C') {   // C Q max_chunk batch lanes max_lanes -> cap n_sub per n_lanes | q0 n lane slot per sub-batch
      int Q, max_chunk, batch, lanes, max_lanes;
      in >> Q >> max_chunk >> batch >> lanes >> max_lanes;
      const PipeCuts c = pipe_cuts(Q, max_chunk, batch, lanes, max_lanes);
      printf("%d %d %d %d |", c.cap, c.n_sub, c.per, c.n_lanes);
      for (int j = 0; j < c.n_sub; ++j) printf(" %d %d %d %d", c.q0(j), c.n(j, Q), c.lane(j), c.slot(j));
      printf("\n");
    } else if (what == 'H') {   // H n_out -> byte offsets of ids, dist, verdict, and the block's bytes
      size_t n_out;
      in >> n_out;
      static char block[4096];
      const HioOut o(block, n_out);
      printf("%td %td %td %zu\n", (char*)o.ids - block, (char*)o.dist - block, (char*)o.verdict - block, HioOut::bytes(n_out));
    }
  }
  return 0;
}
"""

IN_PLACE = 8
ROW300, ROW35 = 1200, 140


# ---- the restatement ----
def m_pieces(Q, pieces):
    if pieces == 1:
        return [(0, Q)]
    per = (-(-Q // pieces) + 31) // 32 * 32
    return [(lo, min(per, Q - lo)) for lo in range(0, Q, per)]


def m_words(row, q_lo, q_hi, n, stage):
    b_lo, b_hi = row * q_lo, row * q_hi
    w0, w1 = b_lo // 16, (b_hi + 15) // 16
    cuts = 4 if (q_lo == 0 and q_hi == n and stage and b_hi >= 512 * 1024) else 1
    per16 = -(-(w1 - w0) // cuts)
    ranges = [(w0 + c * per16, min(w1, w0 + (c + 1) * per16)) for c in range(cuts)]
    return [b_lo, b_hi, w0, w1, cuts, per16, int(b_lo % 16 == 0)], [r for r in ranges if r[0] < r[1]]


def m_source(host, pinned, row, n):
    stage = bool(host and (pinned == 0 or pinned % 16 != 0 or (row * n) % 16 != 0))
    return (n <= IN_PLACE if host else n == 1), stage


def m_cuts(Q, max_chunk, batch, lanes, max_lanes):
    cap = max(1, min(max_chunk, batch))
    n_sub = -(-Q // cap)
    per = -(-Q // n_sub)
    n_lanes = min(n_sub, lanes, max_lanes)
    return [cap, n_sub, per, n_lanes], [(j * per, min(per, Q - j * per), j % n_lanes, (j // n_lanes) & 1) for j in range(n_sub)]


# ---- the cases ----
PIECE_QS = (512, 545, 1024, 1999)
A = 0x7f0000001000          # a pinned buffer's device address: page aligned
# (host, pinned address of the sub-batch's first query, row bytes, n) -> (in_place, stage), named by what then happens
SOURCES = [
    ("in place, pageable staging", (1, 0, ROW300, 8), (True, True)),
    ("in place, pageable staging, the short last sub-batch", (1, 0, ROW300, 2), (True, True)),
    ("in place, the caller's pinned buffer", (1, A + 8 * ROW300, ROW300, 8), (True, False)),
    ("in place, pinned, one query", (1, A, ROW300, 1), (True, False)),
    ("pinned, d = 35, sub-batches of 7 start off a word: staged, in place", (1, A + 7 * ROW35, ROW35, 7), (True, True)),
    ("pinned, d = 35, aligned start but 7 rows end off a word: staged", (1, A, ROW35, 7), (True, True)),
    ("pinned, d = 35, 8 rows from an aligned start: whole words, in place", (1, A + 8 * ROW35, ROW35, 8), (True, False)),
    ("pinned, d = 35, sub-batches of 34 start off a word: staging copy", (1, A + 34 * ROW35, ROW35, 34), (False, True)),
    ("pinned, d = 35, 34 rows end off a word: staging copy", (1, A, ROW35, 34), (False, True)),
    ("pinned, d = 35, the array one row into the buffer: staging copy", (1, A + ROW35, ROW35, 32), (False, True)),
    ("pinned, d = 35, 32 rows from an aligned start: copy kernel from the caller's buffer", (1, A + 68 * ROW35 + 8 * ROW35, ROW35, 32), (False, False)),
    ("one row of a device table where it lies", (0, 0, ROW300, 1), (True, False)),
    ("rows of a device table: gather", (0, 0, ROW300, 25), (False, False)),
    ("rows of a device table, a handful: still a gather", (0, 0, ROW300, 8), (False, False)),
    ("pageable, nine queries: staging copy", (1, 0, ROW300, 9), (False, True)),
    ("pinned, nine queries: copy kernel from the caller's buffer", (1, A, ROW300, 9), (False, False)),
    ("pageable, a whole sub-batch", (1, 0, ROW300, 2048), (False, True)),
]
# (Q, max_chunk, pipeline_batch, pipeline_lanes, max_lanes): the GPU tests' calls, then the edges
CUTS = [(50, 12800, 8, 1, 4), (50, 12800, 8, 4, 4), (49, 12800, 8, 4, 4), (100, 12800, 37, 4, 4), (50, 12800, 40, 4, 4), (1, 12800, 40, 4, 4),
        (2000, 12800, 128, 4, 4), (2000, 12800, 500, 3, 4), (2000, 12800, 333, 1, 4), (2000, 12800, 4096, 4, 4), (1200, 12800, 40, 4, 4),
        (581, 12800, 64, 4, 4), (5000, 1000, 2048, 4, 4), (7, 12800, 0, 4, 4), (9, 12800, 2048, 9, 4), (4096, 12800, 2048, 4, 4)]


def _questions():
    rng = np.random.default_rng(16)
    qs = []
    for Q in PIECE_QS + (1, 31, 32, 33, 127, 128, 511, 2048):
        for pieces in (1, 4):
            qs.append(("P", Q, pieces))
    for Q in PIECE_QS:
        for stage in (0, 1):
            qs += [("W", ROW300, lo, lo + n, Q, stage) for lo, n in m_pieces(Q, 4)]
    # the whole sub-batch in one piece: four copy launches from 512 KiB of staged floats on (436 / 437 queries of 300 dimensions)
    qs += [("W", ROW300, 0, Q, Q, stage) for Q in (1, 8, 9, 436, 437, 512, 2048, 12800) for stage in (0, 1)]
    qs += [("W", ROW35, 0, 34, 34, 1), ("W", ROW35, 0, 7, 7, 1), ("W", ROW35, 7, 14, 14, 1), ("W", ROW35, 4, 8, 8, 0), ("W", 4, 0, 3, 3, 1)]
    qs += [("S",) + c for _, c, _ in SOURCES]
    qs += [("S", int(rng.integers(0, 2)), int(rng.choice([0, A, A + 4, A + 16, A + 140])), int(rng.choice([4, 140, 256, 1200])), int(rng.integers(1, 40))) for _ in range(200)]
    qs += [("C",) + c for c in CUTS]
    qs += [("C", int(rng.integers(1, 5000)), int(rng.integers(1, 3000)), int(rng.integers(1, 3000)), int(rng.integers(1, 6)), 4) for _ in range(200)]
    qs += [("H", n) for n in (1, 5, 10, 320)]
    return qs


def _answer(q):
    """the line the program must print for question q"""
    if q[0] == "P":
        return "".join(f"{lo} {n} " for lo, n in m_pieces(q[1], q[2])) + "| 0"
    if q[0] == "W":
        head, ranges = m_words(*q[1:])
        return " ".join(map(str, head)) + " |" + "".join(f" {a} {b}" for a, b in ranges)
    if q[0] == "S":
        in_place, stage = m_source(*q[1:])
        return f"{int(in_place)} {int(stage)}"
    if q[0] == "C":
        head, subs = m_cuts(*q[1:])
        return " ".join(map(str, head)) + " |" + "".join(f" {a} {b} {c} {d}" for a, b, c, d in subs)
    n = q[1]
    return f"0 {4 * n} {8 * n} {8 * n + 16}"


def _build(tmp, name, extra):
    src = tmp / "stage_main.cpp"
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
        assert line.rstrip() == _answer(q).rstrip(), (q, line)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ not on PATH"
    return tmp_path_factory.mktemp("stage_plan")


@pytest.mark.parametrize("Q", PIECE_QS)
def test_pieces_are_whole_tiles_and_tile_the_sub_batch(Q):
    """the restatement's pieces (the program's are compared with them below): whole 32-query tiles, every query in exactly one piece;
    d = 300: every piece starts on a 16-byte word, inner pieces end on one, and the word ranges cover the block once"""
    pieces = m_pieces(Q, 4)
    assert 1 < len(pieces) <= 4
    assert all(lo % 32 == 0 for lo, _ in pieces) and all(n % 32 == 0 and n >= 128 for _, n in pieces[:-1]) and pieces[-1][1] > 0
    covered = np.concatenate([np.arange(lo, lo + n) for lo, n in pieces])
    assert np.array_equal(covered, np.arange(Q))
    at = 0
    for lo, n in pieces:
        head, ranges = m_words(ROW300, lo, lo + n, Q, 1)
        assert head[6] == 1 and head[4] == 1 and head[2] == at and ranges == [(head[2], head[3])]
        assert head[1] % 16 == 0 or lo + n == Q
        at = head[3]
    assert at == (Q * ROW300 + 15) // 16


def test_source_cases_say_what_they_mean():
    for what, case, exp in SOURCES:
        assert m_source(*case) == exp, what
    seen = {m_source(*c) + (bool(c[0]),) for _, c, _ in SOURCES}
    assert seen == {(True, True, True), (True, False, True), (False, True, True), (False, False, True), (True, False, False), (False, False, False)}


def test_cuts_of_the_gpu_tests_calls():
    assert m_cuts(50, 12800, 8, 1, 4) == ([8, 7, 8, 1], [(0, 8, 0, 0), (8, 8, 0, 1), (16, 8, 0, 0), (24, 8, 0, 1), (32, 8, 0, 0), (40, 8, 0, 1), (48, 2, 0, 0)])
    assert m_cuts(49, 12800, 8, 4, 4)[0] == [8, 7, 7, 4] and m_cuts(100, 12800, 37, 4, 4)[0] == [37, 3, 34, 3]
    assert [s[1] for s in m_cuts(100, 12800, 37, 4, 4)[1]] == [34, 34, 32]
    for c in CUTS:
        head, subs = m_cuts(*c)
        assert sum(s[1] for s in subs) == c[0] and all(0 < s[1] <= head[0] for s in subs) and [s[0] for s in subs] == list(np.cumsum([0] + [s[1] for s in subs[:-1]]))


def test_program_equals_the_restatement(tmp):
    _check(_build(tmp, "stage", []))


def test_program_under_the_sanitizers(tmp):
    """the same program built with AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded,
    nothing sanitised is loaded into Python): the same answers, and no report"""
    _check(_build(tmp, "stage_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"]))
