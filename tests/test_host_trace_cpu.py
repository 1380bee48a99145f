"""The host mirror (postgres-word2vec_amd/host/freddy_udf.cpp) without a GPU: it computes no distance, it checks arguments,
resolves ids and forwards to the device through 26 freddy_gpu_* functions.  tests/host_trace/stub_gpu.c defines those 26 as a
recorder (one line per call: scalars, handle ordinals, hashes of every input array; outputs filled from the hashes),
tests/host_trace/trace_main.cpp calls every function of include/freddy_udf.h on its accepting path and through its refusals,
and fails each device call of insert_batch / delete_rows / update_rows in turn.  The output must equal tests/golden/host_trace.txt
byte for byte.  The golden file was recorded from the mirror as it was BEFORE it was split into headers and is never regenerated
from later code: a difference means the mirror changed what it checks, says, sends to the device or emits."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "postgres-word2vec_amd", "host")
HERE = os.path.join(ROOT, "tests", "host_trace")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_trace.txt")


def _makefile_flags(name):
    text = open(os.path.join(HOST, "Makefile")).read().replace("\\\n", " ")
    return re.search(r"^%s\s*=\s*(.*)$" % name, text, re.M).group(1).split()


def _build(out_dir, tag, cxxflags, cflags):
    exe = os.path.join(out_dir, "trace_" + tag)
    stub_o = os.path.join(out_dir, "stub_%s.o" % tag)
    subprocess.check_call(["gcc"] + cflags + ["-c", os.path.join(HERE, "stub_gpu.c"), "-o", stub_o])
    subprocess.check_call(["g++"] + cxxflags + ["-o", exe, os.path.join(HERE, "trace_main.cpp"), os.path.join(HOST, "freddy_udf.cpp"), stub_o])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The driver + stub + host mirror, once with the flags of host/Makefile and once with its sanitizer flags (built side by side)."""
    out = str(tmp_path_factory.mktemp("host_trace"))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    sanflags = _makefile_flags("SANFLAGS")
    assert all(f in sanflags for f in san)
    with ThreadPoolExecutor(2) as pool:
        plain = pool.submit(_build, out, "plain", _makefile_flags("CXXFLAGS"), ["-O2", "-g", "-Wall", "-Wextra"])
        # the sanitizer runtimes linked statically: the program then does not depend on being first in the list of loaded libraries
        asan = pool.submit(_build, out, "asan", sanflags + ["-static-libasan", "-static-libubsan"], ["-O1", "-g", "-Wall", "-Wextra"] + san)
        return {"dir": out, "plain": plain.result(), "asan": asan.result()}


def _run(exe, cwd, env=None):
    return subprocess.run([exe], cwd=cwd, env=env, capture_output=True, timeout=120)


def test_host_mirror_trace_equals_the_recorded_one(programs):
    cp = _run(programs["plain"], programs["dir"])
    assert cp.returncode == 0, cp.stderr.decode()[-2000:]
    golden = open(GOLDEN, "rb").read()
    if cp.stdout != golden:
        got, want = cp.stdout.split(b"\n"), golden.split(b"\n")
        i = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        ctx = b"\n".join(want[max(0, i - 6):i]).decode()
        raise AssertionError("trace differs from tests/golden/host_trace.txt at line %d\n...\n%s\nrecorded: %s\nnow:      %s"
                             % (i + 1, ctx, want[i].decode() if i < len(want) else "<end>", got[i].decode() if i < len(got) else "<end>"))
    assert len(golden) < 200 * 1024


def test_host_mirror_trace_under_asan_and_ubsan(programs):
    """All of the host mirror under ASan + UBSan with leak detection: a stand-alone program, run directly (no python loads it,
    nothing is preloaded for it).  Every handle the mirror pins it must unpin exactly once."""
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    cp = _run(programs["asan"], programs["dir"], env)
    err = cp.stderr.decode()
    assert cp.returncode == 0, err[-3000:]
    assert "AddressSanitizer" not in err and "LeakSanitizer" not in err and "runtime error:" not in err, err[-3000:]
    assert cp.stdout == open(GOLDEN, "rb").read()
    assert b"DOUBLE UNPIN" not in cp.stdout
    assert cp.stdout.endswith(b"live handles: 0\n")
