"""GPU-box helper: the exact kNN-join (exact_join.h) against the all-exact subset path it replaces, at 3 M x 300.

Two worker processes pin the same table: "join" calls freddy_gpu_exact_join of this build, "parent" calls
freddy_gpu_exact_search(subset) of the library EXACT_JOIN_PARENT_SO names (a build of the parent commit; without it, this build's
own exact_search, whose subset routing the join does not change).  The driver alternates them call group by call group on one box
(the A/B method of tools/lab) and reports medians:
  main     5 000 queries x 100 000 targets, k = 5: both medians, the ratio, per-kernel times, candidates per query, redone queries
  tiles    the same call with 64-query tiles (option exact_join_tile = 64) beside the default 128
  sweep    n_targets in {1 k, 4 k, 8 k, 32 k, 100 k, 1 M} x Q in {1, 64, 1024, 5000}, filter forced, against the parent's path
The driver waits on its workers' pipes without a limit of its own: run it under `timeout`.
  timeout 1100 python tools/exact_join_timing.py > profiles/exact_join_timing.txt"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
N = int(os.environ.get("EXACT_JOIN_N", 3_000_000))
CALLS = int(os.environ.get("EXACT_JOIN_CALLS", 20))
K = 5


def worker(role):
    import numpy as np, torch
    from freddy_amd import gpu, index_build as ib
    parent_so = os.environ.get("EXACT_JOIN_PARENT_SO") if role == "parent" else None
    if parent_so:   # (the parent commit's library has no join entry points; this worker never calls them)
        gpu.load(os.path.abspath(parent_so), optional=("freddy_gpu_exact_join", "freddy_gpu_last_exact_join_stats"))
    x = ib.make_corpus(N, seed=11, device=torch.device("cuda", 0)).cpu().numpy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    idx = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(0)
    qs_all = x[rng.choice(N, 5000, replace=False)].copy()
    t_all = ids[rng.permutation(N)[:1_000_000]].copy()
    print(json.dumps({"ready": role, "N": N, "d": int(x.shape[1])}), flush=True)
    for line in sys.stdin:
        c = json.loads(line)
        qs, t = qs_all[:c["Q"]], t_all[:c["nT"]]
        if role == "join":
            idx.set_option("exact_filter", c.get("filter", -1))
            idx.set_option("exact_join_tile", c.get("tile", 0))
            call = lambda: idx.join(qs, K, t)   # noqa: E731
        else:
            call = lambda: idx.search(qs, K, subset_ids=t)   # noqa: E731
        for _ in range(c.get("warm", 1)):
            call()
        if c.get("profile"):
            idx.profile_enable(True)
        ms = []
        for _ in range(c["calls"]):
            t0 = time.perf_counter()
            gi, gs = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec = {"ms": ms, "crc": int(gi.astype(np.int64).sum() % 1000003), "sim_crc": int(gs.view(np.uint32).astype(np.int64).sum() % 1000003)}
        if c.get("profile"):
            rec["kernels_ms_per_call"] = {k: round(v[1] / c["calls"], 3) for k, v in idx.profile_read().items()}
            idx.profile_enable(False)
        if role == "join":
            rec["stats"] = idx.last_join_stats()
            rec["bound_violations"] = idx.bound_violations()
        print(json.dumps(rec), flush=True)


class Worker:
    def __init__(self, role, env):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", role], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        self.info = None

    def ready(self):
        self.info = json.loads(self.p.stdout.readline())
        return self

    def run(self, **c):
        self.p.stdin.write(json.dumps(c) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("worker ended")
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def alternate(a, b, groups, per_group, **c):
    """groups x (per_group calls of a, per_group calls of b): the medians over all calls of each side, and the last records."""
    ma, mb, ra, rb = [], [], None, None
    for _ in range(groups):
        ra = a.run(calls=per_group, **c); ma += ra["ms"]
        rb = b.run(calls=per_group, **c); mb += rb["ms"]
    return statistics.median(ma), statistics.median(mb), ra, rb


def main():
    env = dict(os.environ)
    parent_so = os.environ.get("EXACT_JOIN_PARENT_SO")
    j, p = Worker("join", env), Worker("parent", env)   # (both tables are built and pinned side by side)
    j.ready(); p.ready()
    out = {"N": j.info["N"], "d": j.info["d"], "k": K, "parent_library": "parent commit build" if parent_so else "this build's exact_search(subset)"}
    per = 5
    mj, mp, rj, rp = alternate(j, p, max(1, CALLS // per), per, Q=5000, nT=100_000, profile=True)
    assert (rj["crc"], rj["sim_crc"]) == (rp["crc"], rp["sim_crc"]), "join and parent lists differ"
    out["main_Q5000_T100000"] = {"join_median_ms": round(mj, 3), "parent_median_ms": round(mp, 3), "join_over_parent": round(mj / mp, 4), "speedup": round(mp / mj, 2),
                                 "join_kernels_ms_per_call": rj["kernels_ms_per_call"], "parent_kernels_ms_per_call": rp["kernels_ms_per_call"],
                                 "candidates_per_query": round(rj["stats"]["candidates"] / 5000, 1), "redone_queries": rj["stats"]["redone_queries"],
                                 "bound_violations": rj["bound_violations"], "calls_per_side": len(rj["ms"]) * max(1, CALLS // per)}
    print("main", json.dumps(out["main_Q5000_T100000"]), flush=True)
    t64 = j.run(calls=CALLS, Q=5000, nT=100_000, tile=64, profile=True)
    out["tile64_Q5000_T100000"] = {"join_median_ms": round(statistics.median(t64["ms"]), 3), "kernels_ms_per_call": t64["kernels_ms_per_call"]}
    print("tile64", json.dumps(out["tile64_Q5000_T100000"]), flush=True)
    sweep = {}
    for nT in (1000, 4000, 8000, 32000, 100_000, 1_000_000):
        for Q in (1, 64, 1024, 5000):
            n = 2 if nT * Q >= 1_000_000_000 else 5
            mj, mp, rj, rp = alternate(j, p, 2, n, Q=Q, nT=nT, filter=1)
            assert (rj["crc"], rj["sim_crc"]) == (rp["crc"], rp["sim_crc"]), ("lists differ", nT, Q)
            sweep[f"T{nT}_Q{Q}"] = {"join_ms": round(mj, 3), "parent_ms": round(mp, 3), "join_over_parent": round(mj / mp, 3),
                                    "candidates_per_query": round(rj["stats"]["candidates"] / Q, 1), "redone_queries": rj["stats"]["redone_queries"]}
            print(f"T{nT}_Q{Q}", json.dumps(sweep[f"T{nT}_Q{Q}"]), flush=True)
    out["sweep_filter_forced"] = sweep
    out["bound_violations"] = rj["bound_violations"]
    j.close(); p.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        main()
