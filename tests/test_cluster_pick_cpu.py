"""include/freddy_pick.h -- the rank generic_cluster draws, shared by the host compiler and the device compiler -- against the
nearbyint form the host mirror had.  tests/cluster_pick_check.c is a program of its own: built plain, and built with ASan + UBSan
(their runtimes linked into it) and run as it is."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("kind", ["plain", "asan_ubsan"])
def test_pick_equals_the_nearbyint_form(kind, tmp_path):
    """For u in {1, 2, 3, 10, 4096, 2^31 - 1}: the draws 0 and 1 - 2^-53, the exact halves with even and odd integer parts, 10^6 random
    draws, and draws outside [0, 1) (clamped before any conversion to int)."""
    exe = str(tmp_path / ("cluster_pick_check_" + kind))
    flags = ["-O2"]
    if kind == "asan_ubsan":
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                 "-static-libasan", "-static-libubsan"]
    subprocess.check_call(["gcc"] + flags + ["-std=c11", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe,
                                             "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cluster_pick_check.c"), "-lm"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = p.stdout.splitlines()
    assert p.returncode == 0, "freddy_pick.h differs from nearbyint (mismatches, first draw's bits, u):\n" + p.stdout[-2000:] + p.stderr[-3000:]
    assert len(lines) == 6 and all(ln.startswith("0 ") for ln in lines), p.stdout
