"""Codegen guard of the front kernel of the kNN-join by row id (join_kernels.h sub_dist_rows_kernel), test_codegen.py's probe with
ceilings of its own (tests/golden/join_ids_codegen_ceilings.json): a gather of half a row into LDS and the join's query block, then
sub_dist_kernel's loop with fifteen loads in flight.  It may not spill or touch scratch, and its registers and occupancy stay within
what the build gave when it was written.  Registers, spills and occupancy only."""
import json
import os
import shutil

import pytest

import test_codegen as tc

CEILINGS = os.path.join(tc.ROOT, "tests", "golden", "join_ids_codegen_ceilings.json")
PROBES = {
    "sub_dist_rows_kernel": ("join.h", "sub_dist_rows_kernel", "sub_dist_rows_kernel"),
}


def measure(tmp):
    saved = tc.PROBES
    tc.PROBES = PROBES            # (probe() reads the table by name)
    try:
        return {n: tc.probe(n, tmp) for n in PROBES}
    finally:
        tc.PROBES = saved


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None, reason="hipcc not on PATH")
def test_the_front_kernel_does_not_spill_and_stays_within_its_registers(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    bad = []
    for name, g in got.items():
        c = ceilings[name]
        for k in ("vgpr_spill", "sgpr_spill", "scratch_bytes"):
            if g[k] != 0:
                bad.append(f"{name}: {k} = {g[k]}, must be 0")
        for k in ("vgprs", "agprs"):
            if g[k] > c[k]:
                bad.append(f"{name}: {k} = {g[k]} > ceiling {c[k]}")
        if g["occupancy"] < c["occupancy"]:
            bad.append(f"{name}: occupancy = {g['occupancy']} waves/SIMD < {c['occupancy']}")
    assert not bad, "\n".join(bad) + "\n(measured: " + json.dumps(got) + ")"


if __name__ == "__main__":   # python tests/test_join_ids_codegen.py [--write]: print (and commit) today's figures
    import sys
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
