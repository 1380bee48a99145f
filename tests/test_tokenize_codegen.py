"""Codegen guard of the text-vector kernels (csrc/tokenize.h), test_codegen.py's probe with ceilings of their own
(tests/golden/tokenize_codegen_ceilings.json): the resolve, the row lists, the centroid with TOK_AHEAD rows of two units in flight
per lane (sixteen 16-byte loads ahead of the adds in the float4 form), and both forms of the normalisation.  None may spill or
touch scratch, and registers and occupancy stay within what the build gave when they were written."""
import json
import os
import shutil

import pytest

import test_codegen as tc

CEILINGS = os.path.join(tc.ROOT, "tests", "golden", "tokenize_codegen_ceilings.json")
PROBES = {
    "tok_resolve_kernel": ("tokenize.h", "tok_resolve_kernel", "tok_resolve_kernel"),
    "tok_rows_kernel": ("tokenize.h", "tok_rows_kernel", "tok_rows_kernel"),
    "tok_centroid_kernel<float4>": ("tokenize.h", "tok_centroid_kernel<float4>", "tok_centroid_kernelI15HIP_vector_type"),
    "tok_centroid_kernel<float>": ("tokenize.h", "tok_centroid_kernel<float>", "tok_centroid_kernelIfE"),
    "tok_unit_kernel<float4>": ("tokenize.h", "tok_unit_kernel<float4>", "tok_unit_kernelI15HIP_vector_type"),
    "tok_unit_kernel<float>": ("tokenize.h", "tok_unit_kernel<float>", "tok_unit_kernelIfE"),
    "tok_unit_wave_kernel": ("tokenize.h", "tok_unit_wave_kernel", "tok_unit_wave_kernel"),
}


def measure(tmp):
    saved = tc.PROBES
    tc.PROBES = PROBES            # (probe() reads the table by name)
    try:
        return {n: tc.probe(n, tmp) for n in PROBES}
    finally:
        tc.PROBES = saved


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None, reason="hipcc not on PATH")
def test_the_tokenize_kernels_do_not_spill_and_stay_within_their_registers(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    assert set(got) == set(ceilings)
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


if __name__ == "__main__":   # python tests/test_tokenize_codegen.py [--write]: print (and commit) today's figures
    import sys
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
