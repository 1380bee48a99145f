"""GPU-box helper: option exact_filter_k (csrc/exact_rank.h) against the all-exact scan on the SAME handle and build.
3 M x 300 random rows (and 1 M x 1024 under option exact_wide), Q in {1, 64, 1024}, k in {33, 100, 256, 1024}: the option at 32 (the
parent's path, launch for launch) and at 1024 alternated within ONE process over several rounds, equal lists asserted before
anything is timed.  Per shape: ms per call both ways (the median of every round's calls, the median over the rounds, the spread
(max - min) / median of the baseline's rounds -- a difference inside it is no difference), the chain's launches from the handle's
profile (device events around each launch, us per launch), the same with option exact_rank_hist = 1 for the threshold, and the
candidates per query: counted here, from an fp32 product and the plan's strided sample, not read from the kernels.
  exact_filter_k_timing.py            N / ROUNDS / REPS_S / SHAPES ("300,1024") from the environment for a smaller run
  exact_filter_k_timing.py --base     k = 5 and 32, Q = 1 and 64 on 3 M x 300: this tree's library against FREDDY_BASE_SO (a build of
                                      the parent commit), a fresh process per variant and round, alternated; appended to the same file"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ROUNDS, REPS_S = int(os.environ.get("N", 3000000)), int(os.environ.get("ROUNDS", 3)), float(os.environ.get("REPS_S", 0.1))
SHAPES = [int(v) for v in os.environ.get("SHAPES", "300,1024").split(",")]
OUT = os.path.join(ROOT, "profiles", "exact_filter_k_timing.txt")
med = statistics.median
fmt = lambda v: "/".join(f"{t:.3f}" for t in v)


def timed(call):
    call()
    t = time.perf_counter(); call(); one = time.perf_counter() - t
    ts = [one]
    for _ in range(int(min(200, max(2, REPS_S / max(one, 1e-6))))):
        t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)   # (every call is synchronous)
    return med(ts) * 1e3


def table(d):
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
    from freddy_amd import gpu
    gpu.load()
    rows = N if d <= 512 else min(N, 1000000)
    xd = torch.randn(rows, d, generator=torch.Generator(device="cuda").manual_seed(d), device="cuda")
    xh = xd.cpu().numpy()
    qs = np.ascontiguousarray(xh[np.random.default_rng(d).choice(rows, 1024, replace=False)]) + np.float32(0.05)
    vec = gpu.VectorIndex(np.arange(1, rows + 1, dtype=np.int32), xh)
    if d > 512:
        vec.set_option("exact_wide", 1)
    return vec, xd, qs


def candidates(xd, qs, k):
    """per query, rows with a >= tau - 2 eps: a = the fp32 product, tau = the k-th best of exact_host.h's filter_plan_k sample"""
    import torch
    rows, d = xd.shape
    strips = rows // 32
    n_sample = min(strips, 32768 * min(8, (k + 31) // 32) // 32) * 32
    stride = max(1, strips // (n_sample // 32))
    a = xd @ torch.from_numpy(qs).cuda().T
    sample = a[:strips * 32].view(strips, 32, -1)[::stride][:n_sample // 32].reshape(n_sample, -1)
    tau = sample.topk(k, dim=0).values[-1]
    eps = (4e-5 if d <= 300 else 1.1e-4) * xd.norm(dim=1).max() * torch.from_numpy(qs).cuda().norm(dim=1)
    return (a >= tau - 2 * eps).sum(dim=0).float().mean().item(), n_sample


def main(say):
    import numpy as np
    say(f"# exact kNN, option exact_filter_k = 1024 (filter) against 32 (scan: the all-exact kernels, the parent's path); ms per call: the median of each")
    say(f"# round's calls, {ROUNDS} rounds, one process, the two alternated inside every round.  spread: (max - min) / median of scan's own rounds.")
    say("# us per launch from the profile: sample / threshold (exact_threshold_rank; [hist4]: option exact_rank_hist = 1) / filter / refine.  cand: candidates per")
    say("# query (counted by the tool, mean of <= 64 queries); sample: rows of the threshold sample")
    say(f"#    d       rows     Q     k  {'scan':>9s} {'filter':>9s}   spread  filter/scan   sample  thr [hist4]  filter   refine     cand   sample   rounds: scan | filter")
    for d in SHAPES:
        vec, xd, qs = table(d)
        labels = ["exact_sample", "exact_threshold_rank", "exact_filter", "exact_refine"] if d <= 512 else \
                 ["exact_sample_wide", "exact_threshold_rank", "exact_filter_wide", "exact_refine"]
        for Q in (1, 64, 1024):
            for k in (33, 100, 256, 1024):
                q = qs[:Q]
                vec.set_option("exact_filter_k", 32)
                base = vec.search(q, k)
                vec.set_option("exact_filter_k", 1024)
                got = vec.search(q, k)
                assert np.array_equal(base[0], got[0]) and np.array_equal(base[1].view(np.uint32), got[1].view(np.uint32)), (d, Q, k)
                res = {"scan": [], "filter": []}
                for _ in range(ROUNDS):
                    for name, value in (("scan", 32), ("filter", 1024)):
                        vec.set_option("exact_filter_k", value)
                        res[name].append(timed(lambda: vec.search(q, k)))
                us, redo = {}, ""
                for hist in (0, 1):
                    vec.set_option("exact_rank_hist", hist)
                    vec.profile_enable(True)
                    for _ in range(5):
                        vec.search(q, k)
                    prof = vec.profile_read()
                    vec.profile_enable(False)
                    redo = "  REDO: a candidate buffer overflowed, the scan answered" if "exact_scan" in prof else redo
                    us[hist] = [prof[n][1] * 1e3 / prof[n][0] for n in labels]
                vec.set_option("exact_rank_hist", 0)
                cand, n_sample = candidates(xd, q[:64], k)
                m = {n: med(v) for n, v in res.items()}
                say(f"{d:6d} {xd.shape[0]:10d} {Q:5d} {k:5d}  {m['scan']:9.3f} {m['filter']:9.3f}   {(max(res['scan']) - min(res['scan'])) / m['scan']:6.3f}  "
                    f"{m['filter'] / m['scan']:11.3f}   {us[0][0]:6.1f} {us[0][1]:5.1f} [{us[1][1]:5.1f}] {us[0][2]:7.1f} {us[0][3]:8.1f} {cand:8.0f} {n_sample:8d}   "
                    f"{fmt(res['scan'])} | {fmt(res['filter'])}{redo}")
        vec.close()
        del xd


def child():
    vec, _, qs = table(300)
    print(json.dumps({f"Q={Q} k={k}": timed(lambda: vec.search(qs[:Q], k)) for Q in (1, 64) for k in (5, 32)}))


def base(say):
    so = os.environ["FREDDY_BASE_SO"]
    say(f"# k <= 32 (the path the option does not touch), {N} x 300: this tree's library against a build of the parent commit, a fresh process per")
    say(f"# variant and round, alternated; ms per call (median of the process's calls), {ROUNDS} rounds: parent | tree, and the parent's spread")
    res = {"parent": [], "tree": []}
    for _ in range(ROUNDS):
        for name in res:
            env = dict(os.environ, **({"FREDDY_GPU_SO": so} if name == "parent" else {}))
            out = subprocess.run([sys.executable, __file__, "--child"], env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            res[name].append(json.loads(out.strip().splitlines()[-1]))
    for key in res["tree"][0]:
        p, t = [r[key] for r in res["parent"]], [r[key] for r in res["tree"]]
        say(f"  {key:12s} parent {med(p):8.3f}  tree {med(t):8.3f}  tree/parent {med(t) / med(p):6.3f}  spread {(max(p) - min(p)) / med(p):6.3f}   {fmt(p)} | {fmt(t)}")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        with open(OUT, "a" if "--base" in sys.argv else "w") as f:
            def say(line=""):
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            (base if "--base" in sys.argv else main)(say)
