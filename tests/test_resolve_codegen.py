"""Codegen guard of the device resolve's kernels (resolve.h), test_codegen.py's probe with ceilings of its own
(tests/golden/resolve_codegen_ceilings.json): three small kernels -- a binary search and an atomic per lane, a popcount reduction,
a wave prefix and a loop over set bits.  None may spill or touch scratch, and their registers stay within what the build gave when
they were written (all three fit the smallest register budget, so the chip's full occupancy)."""
import json
import os
import shutil

import pytest

import test_codegen as tc

CEILINGS = os.path.join(tc.ROOT, "tests", "golden", "resolve_codegen_ceilings.json")
PROBES = {
    "resolve_mark_kernel": ("resolve.h", "resolve_mark_kernel", "resolve_mark_kernel"),
    "resolve_count_kernel": ("resolve.h", "resolve_count_kernel", "resolve_count_kernel"),
    "resolve_place_kernel": ("resolve.h", "resolve_place_kernel", "resolve_place_kernel"),
}


def measure(tmp):
    saved = tc.PROBES
    tc.PROBES = PROBES            # (probe() reads the table by name)
    try:
        return {n: tc.probe(n, tmp) for n in PROBES}
    finally:
        tc.PROBES = saved


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None, reason="hipcc not on PATH")
def test_resolve_kernels_do_not_spill_and_stay_within_their_registers(tmp_path):
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


if __name__ == "__main__":   # python tests/test_resolve_codegen.py [--write]: print (and commit) today's figures
    import sys
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
