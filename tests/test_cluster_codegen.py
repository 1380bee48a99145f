"""Codegen guard of the clustering kernels (csrc/cluster.h), test_codegen.py's probe with ceilings of its own
(tests/golden/cluster_codegen_ceilings.json): cluster_sample_kernel keeps eight ballot masks, ten ranks and ten rows beside the
walk's counts -- no kernel may spill or touch scratch, and their registers stay within what the build gave when they were written."""
import json
import os
import shutil

import pytest

import test_codegen as tc

CEILINGS = os.path.join(tc.ROOT, "tests", "golden", "cluster_codegen_ceilings.json")
PROBES = {
    "cluster_init_kernel": ("cluster.h", "cluster_init_kernel", "cluster_init_kernel"),
    "cluster_apply_kernel": ("cluster.h", "cluster_apply_kernel", "cluster_apply_kernel"),
    "cluster_sample_kernel": ("cluster.h", "cluster_sample_kernel", "cluster_sample_kernel"),
}


def measure(tmp):
    saved = tc.PROBES
    tc.PROBES = PROBES            # (probe() reads the table by name)
    try:
        return {n: tc.probe(n, tmp) for n in PROBES}
    finally:
        tc.PROBES = saved


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None, reason="hipcc not on PATH")
def test_cluster_kernels_do_not_spill_and_stay_within_their_registers(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    bad = []
    for name, g in got.items():
        c = ceilings[name]
        for k in ("vgpr_spill", "scratch_bytes"):
            if g[k] != 0:
                bad.append(f"{name}: {k} = {g[k]}, must be 0")
        for k in ("vgprs", "agprs", "sgpr_spill"):
            if g[k] > c[k]:
                bad.append(f"{name}: {k} = {g[k]} > ceiling {c[k]}")
        if g["occupancy"] < c["occupancy"]:
            bad.append(f"{name}: occupancy = {g['occupancy']} waves/SIMD < {c['occupancy']}")
    assert not bad, "\n".join(bad) + "\n(measured: " + json.dumps(got) + ")"


if __name__ == "__main__":   # python tests/test_cluster_codegen.py [--write]: print (and commit) today's figures
    import sys
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
