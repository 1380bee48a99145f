"""The grid plan (postgres-word2vec_amd/csrc/grid_plan.h) on its own: every grid and every choice of a kernel that the library
makes from the handle's CU count, as pure functions of (n_cus, work sizes, options).

grid_plan.h is plain C++ (no HIP): compiled here with g++ into a small program with its own main, once as it is and once with
-fsanitize=address,undefined, as test_block_plan_cpu.py compiles the block plan.  Both programs read "formula arguments" lines from
stdin and print one integer per line; every figure is compared with the two numpy restatements of tests/grid_inputs.py -- the
expressions as the .hip files had them before the header existed (PARENT) and as the header has them (PLAN):
  * over a sweep of n_cus in {1, 2, 3, 7, 32, 256, 304} and work sizes at both sides of every min and max;
  * for every GPU case of tests/test_gpu_grid_cus.py (grid_inputs.cases()): at the case's grid_cus values the grid is smaller than
    its work by the stated factor -- the loop the case is about iterates -- and at 256 the grid is the parent's."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import grid_inputs as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "grid_plan.h"
using namespace freddy;
// stdin: one call per line, "formula a b c ...".  stdout: its value, or "?" for a formula the program does not know.
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string f;
    in >> f;
    std::vector<long long> a;
    for (long long v; in >> v;) a.push_back(v);
    a.resize(8, 0);
    long long r = 0;
    if (f == "grid_cus") r = grid_cus_value(a[0], (int)a[1]);
    else if (f == "own") r = filter_scan_own((int)a[0], (int)a[1], (int)a[2], (size_t)a[3]);
    else if (f == "cap") r = filter_scan_cap((int)a[0], (int)a[1], (int)a[2], (int)a[3]);
    else if (f == "persist") r = filter_scan_persist(a[0] != 0, (unsigned)a[1], (int)a[2], (size_t)a[3]);
    else if (f == "sparse_grid") r = sparse_grid((int)a[0], (int)a[1], (int)a[2], (size_t)a[3], a[4] != 0);
    else if (f == "sparse_rule") r = sparse_by_itself((int)a[0], (int)a[1], (int)a[2]) ? 1 : 0;
    else if (f == "spec2") r = spec2_grid((int)a[0], (size_t)a[1]);
    else if (f == "multi") r = multi_grid((int)a[0], (size_t)a[1], (size_t)a[2]);
    else if (f == "ivf_one") r = ivf_one_groups((int)a[0], (int)a[1]);
    else if (f == "pq_one") r = pq_one_groups((int)a[0], (int)a[1], a[2], (int)a[3]);
    else if (f == "rpt") r = assign_pq_rpt((int)a[0], a[1], (int)a[2]);
    else if (f == "filter_grid") r = filter_grid((int)a[0], a[1]);
    else if (f == "join_gx") r = exact_join_gx((int)a[0], a[1], (int)a[2]);
    else if (f == "stats") r = table_stats_grid((int)a[0], a[1]);
    else if (f == "sim_split") r = sim_split((int)a[0], (int)a[1], (int)a[2]);
    else if (f == "sim_tiles") r = sim_tiles_per_wg((int)a[0], (int)a[1], (int)a[2]);
    else if (f == "sim_grid_y") r = sim_grid_y((int)a[0], (int)a[1], (int)a[2]);
    else { printf("?\n"); continue; }
    printf("%lld\n", r);
  }
  return 0;
}
"""

CUS = gi.SWEEP_CUS


def _around(*values):
    """every value, one below and one above (positive ones only)"""
    return sorted({v + e for v in values for e in (-1, 0, 1) if v + e > 0})


def _sweep():
    """(formula, args) with work sizes at both sides of every min and max of the formula, for every n_cus of the sweep"""
    calls = []
    for v in (-5, 0, 1, 2, 255, 256, 257, 304, 10**6):
        for dev in (1, 64, 256, 304):
            calls.append(("grid_cus", (v, dev)))
    for n in CUS:
        for share, reserve in itertools.product((0, 1, 2, 4, 8, 9), (0, 1, 8, 40, 300)):
            sc = max(n // max(1, share), min(n, 32)) - reserve
            for mg in _around(1, max(1, sc), n, 57):
                calls.append(("own", (n, share, reserve, mg)))
            for sp_cap, pairs in itertools.product(_around(1, max(1, sc) * 3, max(1, sc) * 6, 48), (0, 1)):
                calls.append(("sparse_grid", (n, share, reserve, sp_cap, pairs)))
            for el in (0, 1, 64, n):
                calls.append(("cap", (n, el, reserve, max(1, share))))
        for elastic, n_own, cap in itertools.product((0, 1), _around(1, n), (-63, 0, 1, n - 64, n, n + 1)):
            for mg in _around(1, n_own, max(1, cap)):
                calls.append(("persist", (elastic, n_own, cap, mg)))
        for C in (1, 32, 200, 3000):
            for n_items in _around(1, 4 * C, 16 * n):
                calls.append(("sparse_rule", (n, n_items, C)))
        for mg in _around(1, n, 2 * n):
            calls.append(("spec2", (n, mg)))
            for lds in (4096, 43104, 75 * 1024, 75 * 1024 + 1, 150 * 1024, 150 * 1024 + 1, 160 * 1024):   # two, one, and "none" (one) workgroups per CU
                calls.append(("multi", (n, mg, lds)))
        for L in (2, 10, 28, 29, 64, 1024, 4000, 8000):   # 7168 / L on both sides of 256, and of n (down to the max(1, .))
            calls.append(("ivf_one", (n, L)))
            for n_blocks in _around(1, 8, 64, 79, 8 * n, 8 * 256):
                calls.append(("pq_one", (n, L, n_blocks, gi.ONE_WAVES)))
        for targets in _around(1, n * 2 * 4 * gi.AS_PQ_WG):
            calls.append(("rpt", (n, targets, gi.AS_PQ_WG)))
        for rows in _around(1, 256, 2 * n * 256, 8232, 131072):
            calls.append(("filter_grid", (n, rows)))
            for qtiles in (1, 2, 3, 4, 2 * n, 2 * n + 1):
                calls.append(("join_gx", (n, rows, qtiles)))
        for rows in _around(1, 4, 32 * n, 32 * n + 4):
            calls.append(("stats", (n, rows)))
        for n_tiles, nblk in itertools.product(_around(1, 2, 13, 16 * n), _around(1, 4, 18, 16 * n)):
            for f in ("sim_split", "sim_tiles", "sim_grid_y"):
                calls.append((f, (n, n_tiles, nblk)))
    return calls


def _case_calls():
    calls = []
    for c in gi.cases():
        for n in c["cus"] + (gi.DEVICE_CUS,):
            calls.append((c["fn"], (n,) + c["args"]))
    return calls


def _build(tmp, name, extra):
    src = tmp / "grid_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)] + extra, check=True)
    return exe


def _run(exe, calls):
    run = subprocess.run([str(exe)], input="".join(f + " " + " ".join(str(int(v)) for v in a) + "\n" for f, a in calls), capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-4000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(calls) and "?" not in lines
    return [int(v) for v in lines]


def _check(exe):
    calls = _sweep() + _case_calls()
    got = _run(exe, calls)
    for (f, a), g in zip(calls, got):
        assert g == gi.PARENT[f](*a), ("parent", f, a, g, gi.PARENT[f](*a))
        assert g == gi.plan(f, *a), ("plan", f, a, g, gi.plan(f, *a))
    # every formula was asked, at every n_cus of the sweep
    assert {f for f, _ in calls} == set(gi.PLAN) == set(gi.PARENT)
    # the GPU cases, from the program's own figures
    fig = {c: g for c, g in zip(calls, got)}
    for c in gi.cases():
        work = c["work_min"] if c["work_min"] is not None else _sparse_work()
        for n in c["cus"]:
            grid = fig[(c["fn"], (n,) + c["args"])]
            assert work >= c["factor"] * grid * c["per"], (c["name"], n, grid, work)
        assert fig[(c["fn"], (gi.DEVICE_CUS,) + c["args"])] == c["at256"], (c["name"], fig[(c["fn"], (gi.DEVICE_CUS,) + c["args"])], c["at256"])


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not on PATH")
    return tmp_path_factory.mktemp("grid_plan")


def _sparse_work():
    t = gi.sparse_tables()
    return gi.thin_units(t["coarse"], gi.sparse_queries(), gi.SPARSE["W"])


def test_the_two_restatements_agree_and_the_sweep_reaches_both_sides():
    """PARENT and PLAN give the same figure for every call of the sweep, and for every formula the sweep holds calls on both sides
    of its min / max: more than one value comes out at one n_cus (else a formula stuck on one arm would pass unnoticed)."""
    calls = _sweep()
    by = {}
    for f, a in calls:
        assert gi.PARENT[f](*a) == gi.plan(f, *a), (f, a)
        if f not in ("grid_cus", "persist"):
            by.setdefault((f, a[0]), set()).add(gi.plan(f, *a))
    for (f, n), values in by.items():
        # (one CU: min(work, 1) has one value; the two values of rpt are asked for below)
        assert len(values) >= 2 or f == "rpt" or (n == 1 and f in ("own", "spec2", "ivf_one", "pq_one")), (f, n, values)
    assert {gi.plan("rpt", n, t, gi.AS_PQ_WG) for n in CUS for t in _around(n * 2048)} == {1, 4}
    assert {gi.plan("grid_cus", v, 256) for v in (-5, 0, 1, 255, 256, 257, 10**6)} == {256, 1, 255}
    assert {gi.plan("persist", e, 3, c, 100) for e in (0, 1) for c in (-63, 2, 7)} == {3, 7}


def test_gpu_cases_state_what_they_reach():
    """what the GPU cases rely on beyond grid < work: the path choices flip where the cases say, the one-launch kernel's LDS
    fallback, the similarity kernel's ranges"""
    s = gi.SPARSE
    items = s["Q"] * s["W"]
    assert items == 48
    assert [gi.plan("sparse_rule", n, items, s["C"]) for n in (1, 2, 3, 7, 256)] == [1, 1, 1, 0, 0]
    assert _sparse_work() >= 2 * gi.plan("sparse_grid", 3, 1, 0, items, 1) == 18
    # one launch: G < W at grid_cus = 2 (the multi-launch path), G = grid_cus at 3, 7, 13; several units per workgroup (n_slot = 1)
    w = gi.ONE_IVF["W"]
    for L in (10, 64):
        assert [gi.plan("ivf_one", n, L) for n in (2, 3, 7, 13)] == [2, 3, 7, 13] and 2 < w <= 3
        assert all(gi.plan("ivf_one", n, L) < w * gi.ONE_M for n in (3, 7, 13))
        assert gi.plan("ivf_one", 256, L) >= w * gi.ONE_M
        assert gi.ivf_one_lds(gi.ONE_IVF["K"], gi.ONE_IVF["C"], w, L, 3) <= 60 * 1024
        assert gi.ivf_one_lds(gi.ONE_IVF_WIDE["K"], gi.ONE_IVF_WIDE["C"], w, L, 3) > 60 * 1024 >= gi.ivf_one_lds(gi.ONE_IVF_WIDE["K"], gi.ONE_IVF_WIDE["C"], w, L, gi.plan("ivf_one", 256, L))
    # the exact filter: two workgroups at grid_cus = 1, the parent's one strip per wave at 256
    n = gi.EXACT["N"]
    assert gi.plan("filter_grid", 1, n) == 2 and gi.plan("filter_grid", 256, n) * gi.EXF_WAVES >= -(-n // 32)
    # assignment: four targets per thread at grid_cus = 1 with a ragged last workgroup, one per thread at 256
    t = gi.ASSIGN["targets"]
    assert gi.plan("rpt", 1, t, gi.AS_PQ_WG) == 4 and gi.plan("rpt", 2, t, gi.AS_PQ_WG) == 1 and gi.plan("rpt", 256, t, gi.AS_PQ_WG) == 1
    assert t % (4 * gi.AS_PQ_WG) not in (0,) and t > 2 * 4 * gi.AS_PQ_WG
    # similarity: at least three tiles per workgroup with a ragged last range at grid_cus = 1 .. 3, one tile at 256
    sc = gi.sim_cases()
    assert all(tiles == 1 for _, _, n_, tiles, _ in sc if n_ == 256)
    assert any(tiles >= 3 and ragged for _, _, n_, tiles, ragged in sc if n_ == 1)
    assert any(tiles >= 3 and ragged for _, nb, n_, tiles, ragged in sc if n_ == 3 and nb == 1100)
    assert gi.SIM["na"] % gi.SIM_AT != 0
    # table statistics: rows beyond the first sweep of 8 workgroups x 4 rows at grid_cus = 1
    assert gi.plan("stats", 1, gi.STATS["append"]) * 4 == 32


def test_plan_equals_the_restatements(tmp):
    _check(_build(tmp, "grid", []))


def test_plan_under_the_sanitizers(tmp):
    """the same program built with AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded,
    nothing sanitised is loaded into Python): the same figures, and no report"""
    exe = _build(tmp, "grid_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"])
    _check(exe)
