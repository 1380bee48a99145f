"""The layout of the one-launch kernels (postgres-word2vec_amd/csrc/one_layout.h) on its own: from (K, C, W, L, G) the regions of
the hand-off buffer and of the dynamic LDS that pq_one / ivf_one (host) and pq_one_kernel / ivf_one_kernel (device) both read.

one_layout.h is plain C++ (no HIP): compiled here with g++ into a small program with its own main, once as it is and once with
-fsanitize=address,undefined, as test_block_plan_cpu.py compiles the block plan.  Both programs read the same shapes from stdin and
print every offset and extent.  The sweep is K x C x W x k x G below, restricted to what the hosts' shape tests admit (pq_one_shape,
ivf_one_shape, and G's bounds in pq_one / ivf_one: K a multiple of 4 and at most 1024, W <= G <= min(256, 56 KB / 8 L), the 60 KB
refusal of ivf_one); K = 300 is a multiple of 4, so the hosts admit it and it is swept like the others.  Every shape once with
cells (ivf_one) and once without (pq_one: C = 0, one table).  Checked per shape:
  * every hand-off offset, the hand-off size and the dynamic LDS size equal the formulas pq_one and ivf_one carried before the
    header existed, and the LDS offsets equal the pointer arithmetic the kernels carried (restated here in numpy);
  * regions alive in the same stage do not overlap (hand-off: all four; LDS: centroid rows | query, cell distances | cell row,
    table | wave rows, waves' lists | collected lists);
  * every region ends within its total;
  * regions moved with 16-byte loads or stores are 16-byte aligned (tables and distances, in global memory and in LDS; the
    centroid rows and the query), key regions 8-byte aligned."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")
WAVES, M, D = 8, 12, 300
LDS_NAMES = ["coarse_rows", "query", "cell_dist", "cell_row", "table", "wave_rows", "lists", "all_lists"]

PROGRAM = r"""
#include <stdio.h>
#include "one_layout.h"
using namespace freddy;
// stdin: "K C W L G" per line.  stdout per shape: lut_off part_off cnt_off handoff_bytes lds_bytes cells_per_group, then
// (off, bytes) of the LDS regions: coarse_rows query (both for cells_per_group cells) cell_dist cell_row table wave_rows lists all_lists
int main() {
  static_assert(ONE_WG == 512 && ONE_WAVES == 8 && ONE_M == 12 && ONE_D == 300, "the constants the test restates");
  int K, C, W, L, G;
  while (scanf("%d %d %d %d %d", &K, &C, &W, &L, &G) == 5) {
    const OneLayout y{K, C, W, L, G};
    const size_t n = y.cells_per_group();
    printf("%zu %zu %zu %zu %zu %zu", y.lut_off(), y.part_off(), y.cnt_off(), y.handoff_bytes(), y.lds_bytes(), n);
    const OneRegion r[] = {y.coarse_rows(n), y.query(n), y.cell_dist(), y.cell_row(), y.table(), y.wave_rows(), y.lists(), y.all_lists()};
    for (const OneRegion& x : r) printf(" %zu %zu", x.off, x.bytes);
    printf("\n");
  }
  return 0;
}
"""


def _shapes():
    """(K, C, W, L, G) the hosts admit; C = 0: pq_one (W = 1)"""
    out = []
    for K, C, W, k in itertools.product([16, 256, 300, 1024], [1, 8, 100, 4096], [1, 10, 32], [1, 5, 32]):
        L = 2 * k
        if K & 3 or K > 1024 or W > 32 or L > 64 or C > 4096:
            continue
        for G in sorted({1, W, 64, 256}):
            if G > min(256, 56 * 1024 // (8 * L)):
                continue
            if G >= W and _parent(K, C, W, L, G)["lds"] <= 60 * 1024:
                out.append((K, C, W, L, G))
            if W == 1 and C == 1:
                out.append((K, 0, 1, L, G))
    return out


def _up(n, a):
    return (n + a - 1) & ~(a - 1)


def _parent(K, C, W, L, G):
    """the figures as pq_one / ivf_one and the kernels stated them before one_layout.h"""
    lutN = M * K
    scan = max(_up(lutN * 4, 16) + WAVES * 64 * 8, WAVES * 64 * 8 + G * L * 8)
    kernel = dict(wave_rows=_up(lutN * 4, 16), lists=0, all_lists=WAVES * 64 * 8, table=0)
    if C == 0:
        part_off = _up(lutN * 4, 256)
        return dict(lut_off=0, part_off=part_off, bytes=part_off + 8 * G * L, lds=scan, **kernel)
    lut_off = _up(4 * (C + 8), 256)
    part_off = _up(lut_off + 4 * W * lutN, 256)
    cnt_off = _up(part_off + 8 * G * L, 256)
    n_mine = (C + G - 1) // G
    lds = max((n_mine + 1) * D * 4, C * 4 + 64 + 64 * 8 + 64, scan)
    return dict(lut_off=lut_off, part_off=part_off, cnt_off=cnt_off, bytes=cnt_off + 4 * G, lds=lds, n_mine=n_mine,
                coarse_rows=0, query=n_mine * D * 4, cell_dist=0, cell_row=(C * 4 + 63) & ~15, **kernel)


def _disjoint(regions):
    r = sorted(regions)
    return all(a[0] + a[1] <= b[0] for a, b in zip(r, r[1:]))


def _build(tmp, name, extra):
    src = tmp / "one_layout_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)] + extra, check=True)
    return exe


def _check(exe):
    shapes = _shapes()
    run = subprocess.run([str(exe)], input="".join("%d %d %d %d %d\n" % s for s in shapes), capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-4000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(shapes)
    for shape, line in zip(shapes, lines):
        K, C, W, L, G = shape
        v = [int(t) for t in line.split()]
        lut_off, part_off, cnt_off, total, lds, n_mine = v[:6]
        reg = {n: (v[6 + 2 * i], v[7 + 2 * i]) for i, n in enumerate(LDS_NAMES)}
        exp = _parent(*shape)
        # equal to the parent's
        assert (lut_off, part_off, total, lds) == (exp["lut_off"], exp["part_off"], exp["bytes"], exp["lds"]), (shape, line)
        stages = [["table", "wave_rows"], ["lists", "all_lists"]]
        if C:
            assert (cnt_off, n_mine) == (exp["cnt_off"], exp["n_mine"]), (shape, line)
            stages += [["coarse_rows", "query"], ["cell_dist", "cell_row"]]
        for names in stages:
            for n in names:
                assert reg[n][0] == exp[n], (shape, n, line)
                assert reg[n][0] + reg[n][1] <= lds <= (60 * 1024 if C else 64 * 1024), (shape, n, line)   # within the total
            assert _disjoint([reg[n] for n in names]), (shape, names, line)
        # the extents are what the kernels touch
        assert reg["table"][1] == 4 * M * K and reg["wave_rows"][1] == reg["lists"][1] == WAVES * 64 * 8 and reg["all_lists"][1] == 8 * G * L
        if C:
            assert reg["coarse_rows"][1] == n_mine * D * 4 and reg["query"][1] == D * 4 and reg["cell_row"][1] == 64 * 8
            assert reg["cell_dist"][1] == 4 * _up(C, 4)   # (one_stage_tagged moves whole 16-byte words)
        # the hand-off buffer
        hand = [(lut_off, 4 * W * M * K), (part_off, 8 * G * L)]
        if C:
            hand += [(0, 4 * _up(C, 4)), (cnt_off, 4 * G)]
        assert _disjoint(hand) and all(o + n <= total for o, n in hand), (shape, line)
        # alignment: 16-byte loads and stores of tables and distances, 8-byte keys, the 256-byte starts
        assert lut_off % 256 == 0 and part_off % 256 == 0 and (not C or cnt_off % 256 == 0)
        assert (4 * M * K) % 16 == 0   # every one of the W tables starts at a 16-byte word
        for n in ["table"] + (["coarse_rows", "query", "cell_dist"] if C else []):
            assert reg[n][0] % 16 == 0, (shape, n)
        assert (D * 4) % 16 == 0       # every centroid row too
        for n in ["wave_rows", "lists", "all_lists"] + (["cell_row"] if C else []):
            assert reg[n][0] % 8 == 0, (shape, n)
    return len(shapes)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not on PATH")
    return tmp_path_factory.mktemp("one_layout")


def test_sweep_covers_the_shapes():
    """the sweep holds what it is meant to: both kernels, every K, C, W and k of the grid, a grid of one workgroup and the
    largest, the shape whose collected lists decide the LDS size and one whose table does, and the 60 KB refusal bites"""
    s = _shapes()
    ivf = [x for x in s if x[1]]
    assert {x[0] for x in ivf} == {16, 256, 300, 1024} and {x[1] for x in ivf} == {1, 8, 100, 4096}
    assert {x[2] for x in ivf} == {1, 10, 32} and {x[3] for x in s} == {2, 10, 64} and {x[4] for x in s} >= {1, 10, 32, 64, 256}
    assert any(x[1] == 0 for x in s)
    p = [_parent(*x) for x in s]
    assert any(e["lds"] == 8 * 64 * 8 + 8 * x[3] * x[4] for x, e in zip(s, p)) and any(e["lds"] == 48 * x[0] + 4096 for x, e in zip(s, p))
    assert _parent(16, 4096, 1, 2, 1)["lds"] > 60 * 1024 and (16, 4096, 1, 2, 1) not in s
    assert len(s) > 300


def test_layout_equals_the_parents_formulas(tmp):
    assert _check(_build(tmp, "layout", [])) == len(_shapes())


def test_layout_under_the_sanitizers(tmp):
    """the same program built with AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded,
    nothing sanitised is loaded into Python): the same figures, and no report"""
    exe = _build(tmp, "layout_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"])
    _check(exe)
