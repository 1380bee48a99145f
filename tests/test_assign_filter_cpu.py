"""CPU suite of option assign_filter (csrc/assign_filter.h): freddy_gpu_last_assign_stats is declared, exported, listed and bound; the
header documents the option; and test_cluster_codegen.py's guard for the new kernels -- none spills or touches scratch, and each
stays within tests/golden/assign_filter_codegen_ceilings.json, written from the build that added them."""
import json
import os
import re
import shutil

import pytest

import test_codegen as tc

CEILINGS = os.path.join(tc.ROOT, "tests", "golden", "assign_filter_codegen_ceilings.json")
PROBES = {
    "assign_image_kernel": ("assign_filter.h", "assign_image_kernel", "assign_image_kernel"),
    "assign_filter_kernel<4>": ("assign_filter.h", "assign_filter_kernel<4>", "assign_filter_kernelILi4EE"),
    "assign_refine_kernel": ("assign_filter.h", "assign_refine_kernel", "assign_refine_kernel"),
    "assign_redo_kernel": ("assign_filter.h", "assign_redo_kernel", "assign_redo_kernel"),
}


def test_last_assign_stats_is_declared_exported_listed_and_bound():
    import __graft_entry__ as g
    g.build()
    from freddy_amd import gpu
    header = open(os.path.join(tc.ROOT, "include", "freddy_gpu.h")).read()
    assert re.search(r"\bint freddy_gpu_last_assign_stats\s*\(const freddy_gpu_index_t\*", header)
    assert '"assign_filter"' in header[header.index("paths (each has GPU tests"):header.index("int freddy_gpu_set_option")]
    lib = gpu.load()
    assert hasattr(lib, "freddy_gpu_last_assign_stats") and "freddy_gpu_last_assign_stats" in gpu.EXPORTS
    assert callable(gpu.VectorIndex.last_assign_stats)
    out = (gpu.C.c_int64 * 5)()
    assert lib.freddy_gpu_last_assign_stats(None, out) == -1 and b"NULL" in lib.freddy_gpu_last_error()     # FREDDY_E_ARG


def measure(tmp):
    saved = tc.PROBES
    tc.PROBES = PROBES            # (probe() reads the table by name)
    try:
        return {n: tc.probe(n, tmp) for n in PROBES}
    finally:
        tc.PROBES = saved


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None, reason="hipcc not on PATH")
def test_assign_filter_kernels_do_not_spill_and_stay_within_their_registers(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    bad = []
    for name, g in got.items():
        c = ceilings[name]
        bad += [f"{name}: {k} = {g[k]}, must be 0" for k in ("vgpr_spill", "scratch_bytes") if g[k] != 0]
        bad += [f"{name}: {k} = {g[k]} > ceiling {c[k]}" for k in ("vgprs", "agprs", "sgpr_spill") if g[k] > c[k]]
        if g["occupancy"] < c["occupancy"]:
            bad.append(f"{name}: occupancy = {g['occupancy']} waves/SIMD < {c['occupancy']}")
    assert not bad, "\n".join(bad) + "\n(measured: " + json.dumps(got) + ")"


if __name__ == "__main__":   # python tests/test_assign_filter_cpu.py [--write]: print (and commit) today's figures
    import sys
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
