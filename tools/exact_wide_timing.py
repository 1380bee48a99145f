"""GPU-box helper: option exact_wide (csrc/exact_wide.h) against the all-exact scan on the SAME handle and build, k = 5.
Per d in {768, 1024, 1536, 2048}: a random table larger than the Infinity Cache (1 M rows, at most 4 GiB), Q in {1, 64, 1024};
the variants alternated within ONE process over several rounds, equal lists asserted before anything is timed:
  off     exact_wide = 0: exact_scan_kernel (the baseline)
  wide    exact_wide = 1, exact_wide_shape = 0: segments of 8 k-steps, one strip per wave, two workgroups per CU
  ts16    exact_wide_shape = 1: segments of 16 k-steps, one workgroup per CU           (Q = 64 only)
  r2      exact_wide_shape = 2: segments of 8, two strips per wave, one workgroup per CU (Q = 64 only)
and the filter pass alone from the handle's profile (device events around the launch, five calls): the table's bytes over its
time against the HBM peak.  Writes profiles/exact_wide_timing.txt: the median of every round's calls, the medians over the rounds
and the spread (max - min) / median of the baseline's rounds -- a difference inside it is no difference.
  exact_wide_timing.py            N / ROUNDS / REPS_S (seconds of calls per figure and round) / DIMS from the environment for a smaller run"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ROUNDS, REPS_S = int(os.environ.get("N", 1000000)), int(os.environ.get("ROUNDS", 3)), float(os.environ.get("REPS_S", 0.1))
DIMS = [int(v) for v in os.environ.get("DIMS", "768,1024,1536,2048").split(",")]
K, HBM_PEAK, MAX_BYTES = 5, 8.0e12, 4 << 30
SHAPES = {"wide": 0, "ts16": 1, "r2": 2}


def main():
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
    from freddy_amd import gpu
    gpu.load()
    note = lambda what: print(f"[exact_wide_timing] {what}", file=sys.stderr, flush=True)

    def timed(call):
        call()
        t = time.perf_counter(); call(); one = time.perf_counter() - t
        ts = [one]
        for _ in range(int(min(200, max(2, REPS_S / max(one, 1e-6))))):
            t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)   # (every call is synchronous)
        return statistics.median(ts) * 1e3

    out = open(os.path.join(ROOT, "profiles", "exact_wide_timing.txt"), "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")

    med = statistics.median
    fmt = lambda v: "/".join(f"{t:.3f}" for t in v)
    say(f"# exact kNN, option exact_wide against the all-exact scan, k = {K}; ms per call: the median of each round's calls, {ROUNDS} rounds, one process,")
    say("# the variants alternated inside every round.  spread: (max - min) / median of off's own rounds.  wide / ts16 / r2: exact_wide_shape 0 / 1 / 2")
    say("# filter us: exact_filter_wide alone (device events, five calls); of peak: rows * d * 4 bytes over that time against 8 TB/s")
    say(f"#    d       rows     Q   {'off':>9s} {'wide':>9s} {'ts16':>9s} {'r2':>9s}   spread  wide/off   filter us  of peak  same lists   rounds: off | wide")
    for d in DIMS:
        rows = int(min(N, MAX_BYTES // (4 * d)))
        note(f"d = {d}: building {rows} rows")
        g = torch.Generator(device="cuda").manual_seed(d)
        xh = torch.randn(rows, d, generator=g, device="cuda").cpu().numpy()
        torch.cuda.empty_cache()
        ids = np.arange(1, rows + 1, dtype=np.int32)
        qs = np.ascontiguousarray(xh[np.random.default_rng(d).choice(rows, 1024, replace=False)]) + np.float32(0.05)
        vec = gpu.VectorIndex(ids, xh)

        def variant(shape, q):
            def run():
                vec.set_option("exact_wide_shape", shape)
                return timed(lambda: vec.search(q, K))
            return run

        for Q in (1, 64, 1024):
            q = qs[:Q]
            vec.set_option("exact_wide", 0)
            base = vec.search(q, K)
            vec.set_option("exact_wide", 1)
            same = True
            for shape in SHAPES.values():
                vec.set_option("exact_wide_shape", shape)
                got = vec.search(q, K)
                same = same and bool(np.array_equal(base[0], got[0]) and np.array_equal(base[1].view(np.uint32), got[1].view(np.uint32)))
            assert same, (d, Q)
            names = ["wide"] + (["ts16", "r2"] if Q == 64 else [])
            res = {n: [] for n in ["off"] + names}
            for _ in range(ROUNDS):
                vec.set_option("exact_wide", 0)     # (releases the copy; setting it again lays it out: outside the timed calls)
                res["off"].append(timed(lambda: vec.search(q, K)))
                vec.set_option("exact_wide", 1)
                for n in names:
                    res[n].append(variant(SHAPES[n], q)())
            vec.set_option("exact_wide_shape", 0)
            vec.profile_enable(True)
            for _ in range(5):
                vec.search(q, K)
            prof = vec.profile_read()
            vec.profile_enable(False)
            launches, ms = prof["exact_filter_wide"]
            us = ms * 1e3 / launches
            m = {n: med(v) for n, v in res.items()}
            cell = lambda n: f"{m[n]:9.3f}" if n in m else f"{'-':>9s}"
            say(f"{d:6d} {rows:10d} {Q:5d}   {cell('off')} {cell('wide')} {cell('ts16')} {cell('r2')}   {(max(res['off']) - min(res['off'])) / m['off']:6.3f}  "
                f"{m['wide'] / m['off']:8.3f}   {us:9.1f}  {rows * d * 4 / (us * 1e-6) / HBM_PEAK:7.3f}  {str(same):10s}   {fmt(res['off'])} | {fmt(res['wide'])}")
        vec.close()
        del xh
    out.close()


if __name__ == "__main__":
    main()
