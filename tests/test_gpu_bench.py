"""-m gpu: bench.py's plain run and --dump-outputs on a small corpus.  A plain run times exactly --steps steps and prints the
result line alone; its inputs are the same from run to run, so two runs -- and a --full run -- dump the same lists."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--N", "200000", "--C", "100", "--warmup", "2"]


def _bench(cwd, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env, timeout=900,
                       cwd=cwd)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout.rstrip("\n").splitlines()


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("ids", "dist")}


def test_plain_run_and_dumped_outputs(tmp_path):
    lines = _bench(str(tmp_path), *SMALL, "--steps", "7", "--dump-outputs", str(tmp_path / "a"))
    assert len(lines) == 1, lines   # the result line alone: no digest
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "queries/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and "details" not in line
    a = _load(tmp_path / "a")
    assert a["ids"].dtype == np.float64 and a["dist"].dtype == np.float32 and a["ids"].shape == (1024, 5) == a["dist"].shape
    assert (a["ids"][:, 0] >= 1).all() and (np.diff(a["dist"], axis=1) >= 0).all()
    # the same arguments: the same corpus, tables and queries, so the same lists, bit for bit
    _bench(str(tmp_path), *SMALL, "--steps", "7", "--dump-outputs", str(tmp_path / "b"))
    b = _load(tmp_path / "b")
    assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["dist"].view(np.uint32), b["dist"].view(np.uint32))
    # --full: the side measurements around the same timed steps, the oracle's verdict on them, the same lists
    lines = _bench(str(tmp_path), *SMALL, "--steps", "7", "--full", "--cpu-sample", "64", "--no-host-abi", "--dump-outputs",
                   str(tmp_path / "c"))
    full = json.loads(lines[-1])
    assert full["steps"] == 7 and full["cpu_baseline"]["parity_with_gpu_on_sample"] is True and full["config"]["recall_at_5"] > 0
    c = _load(tmp_path / "c")
    assert np.array_equal(a["ids"], c["ids"]) and np.array_equal(a["dist"].view(np.uint32), c["dist"].view(np.uint32))
