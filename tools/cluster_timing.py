"""GPU-box helper: cluster_exact / cluster_pq of the host mirror, this build against the parent commit, on the bench tables (3 M x 300;
flat PQ index m = 12, K = 1024), supplied draws, n in {4096, 100 000, 1 M, 3 M} tokens with k in {10, 100}.

A process binds one library, so every (round, side) is a child process of its own that pins the tables, runs every shape (one warm-up,
then REPS timed calls: their median is that round's figure) and prints one line per shape with a digest of the clusters:

    python tools/cluster_timing.py                       the driver: ROUNDS rounds, "parent" and "this" alternated on this box
    python tools/cluster_timing.py --child <tree>        one round of one side (the driver starts these; <tree> is a checkout with its
                                                         libraries built: this tree, or the parent's under tools/ab_head)

The driver asserts that both builds return equal clusters at every shape before it reports a time, then writes
profiles/cluster_timing.txt: per shape the median over the rounds of each side, the parent's spread between its rounds (max - min),
and the verdict "this <= parent + spread"; then, for this build, the milliseconds of every kernel of one more call per shape (the
handles' event profiles).  The yardstick is the parent, never this build.
ROUNDS (4 at least) / REPS / N / SIZES from the environment for a smaller run."""
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.environ.get("CLUSTER_AB_PARENT", os.path.join(ROOT, "tools", "ab_head"))
N = int(os.environ.get("N", 3000000))
ROUNDS = max(4, int(os.environ.get("ROUNDS", 4)))
REPS = int(os.environ.get("REPS", 3))
SIZES = [int(v) for v in os.environ.get("SIZES", "4096,100000,1000000,3000000").split(",")]
KS = (10, 100)


def child(tree):
    sys.path[:0] = [tree, os.path.join(tree, "postgres-word2vec_amd")]
    import numpy as np
    import torch
    from freddy_amd import gpu, index_build as ib, udf
    have = hasattr(gpu.load(), "freddy_gpu_cluster")
    x = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0))
    xh = x.cpu().numpy()
    # the PQ index is trained with atomics, so two processes build different ones: the first child keeps its own for the others
    kept = os.environ.get("CLUSTER_AB_TABLES", "")
    if kept and os.path.exists(kept):
        pq = dict(np.load(kept))
    else:
        pq = {k: np.asarray(v) for k, v in ib.build_pq_index(x, m=12, K=1024, train_size=100000, iters=10, seed=2).items() if k in ("codebook", "ids", "codes")}
        if kept:
            np.savez(kept, **pq)
    del x
    ids = np.arange(1, N + 1, dtype=np.int32)
    s = udf.Session()
    s.load_vecs_norm(ids, xh)
    s.load_pq(pq["codebook"], pq["ids"], pq["codes"])
    print(f"# {'with' if have else 'without'} freddy_gpu_cluster", flush=True)
    walk = int(os.environ.get("CLUSTER_WALK", 0))                # 1: the plain walk of cluster_sample_kernel (option cluster_walk), this build only
    for n in SIZES:
        rng = np.random.default_rng(n)
        tokens = rng.choice(ids, min(n, N), replace=False).astype(np.int32)
        for k in KS:
            draws = rng.random(k + 9 * k * 10)
            for name in ("cluster_exact", "cluster_pq"):
                fn = getattr(s, name)
                out = fn(tokens, k, draws)                       # warm-up (pins the vectors, sizes the workspaces)
                if have and walk:
                    s.gpu_index("vecs").set_option("cluster_walk", walk)
                ts = []
                for _ in range(REPS if n <= 100000 else max(1, REPS - 1)):
                    t = time.perf_counter(); fn(tokens, k, draws); ts.append(time.perf_counter() - t)
                print(f"RESULT {name} {n} {k} {statistics.median(ts) * 1e3:.3f} {hashlib.sha1(out.tobytes()).hexdigest()[:16]}", flush=True)
                if have:                                         # the kernels of one more call, by the handles' own event profiles
                    prof = {}
                    idxs = [s.gpu_index("vecs")] + ([s.gpu_index("pq")] if name == "cluster_pq" else [])
                    for ix in idxs:
                        ix.profile_enable(True)
                    fn(tokens, k, draws)
                    for ix in idxs:
                        prof.update({nm: ms for nm, (_, ms) in ix.profile_read().items()})
                        ix.profile_enable(False)
                    print(f"KERNELS {name} {n} {k} " + " ".join(f"{nm}={ms:.3f}" for nm, ms in sorted(prof.items())), flush=True)
    s.close()


def driver():
    sides = {"parent": PARENT, "this": ROOT, "plain": ROOT}
    times, digests, kernels, plain = {}, {}, {}, {}
    import tempfile
    tmp = tempfile.TemporaryDirectory()
    tables = os.path.join(tmp.name, "pq_tables.npz")
    for r in range(ROUNDS + 1):
        for side in (("parent", "this") if r < ROUNDS else ("plain",)):      # (one more child of this build at the end: the plain walk)
            t0 = time.time()
            # (a time limit per child; a child that fails ends the run: nothing more is started on the device)
            p = subprocess.Popen(["timeout", "-k", "10", os.environ.get("CHILD_LIMIT", "600"), sys.executable, os.path.abspath(__file__), "--child", sides[side]],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, CLUSTER_WALK="1" if side == "plain" else "0", CLUSTER_AB_TABLES=tables),
                                 text=True)
            seen = []
            for ln in p.stdout:                                   # (echoed as it comes: a round of the parent at 3 M tokens takes minutes)
                seen.append(ln.rstrip("\n"))
                print(f"  {side}: {seen[-1]}", flush=True)
            if p.wait() != 0:
                raise SystemExit(f"round {r} {side}: the child failed")
            (plain if side == "plain" else kernels).update({tuple(ln.split()[1:4]): ln for ln in seen if ln.startswith("KERNELS ")})
            for ln in seen:
                if ln.startswith("RESULT ") and side == "plain":
                    _, name, n, k, ms, dg = ln.split()
                    digests.setdefault((name, int(n), int(k)), set()).add(dg)
                    plain[(name, n, k, "call")] = ms
                elif ln.startswith("RESULT "):
                    _, name, n, k, ms, dg = ln.split()
                    key = (name, int(n), int(k))
                    times.setdefault((side,) + key, []).append(float(ms))
                    digests.setdefault(key, set()).add(dg)
            print(f"# round {r} {side}: {time.time() - t0:.0f} s", flush=True)
    bad = [k for k, v in digests.items() if len(v) != 1]
    assert not bad, f"the two builds (or two rounds) return different clusters at {bad}"
    lines = [f"# cluster_exact / cluster_pq through the host mirror, {N} x 300, PQ m=12 K=1024, supplied draws, one call = ten rounds",
             f"# {ROUNDS} rounds, parent and this build alternated on one box, a process per (round, side); per round the median of {REPS} calls"
             f" ({max(1, REPS - 1)} from 1 M tokens on) after one warm-up; equal clusters asserted at every shape",
             "# function            n    k  parent_ms (spread)      this_ms (spread)   parent/this  this <= parent + spread"]
    slower = []
    for key in sorted(digests, key=lambda c: (c[0], c[1], c[2])):
        pa, th = times[("parent",) + key], times[("this",) + key]
        pm, tm = statistics.median(pa), statistics.median(th)
        ps, tsp = max(pa) - min(pa), max(th) - min(th)
        ok = tm <= pm + ps
        if not ok:
            slower.append(key)
        lines.append(f"{key[0]:14s} {key[1]:8d} {key[2]:4d}  {pm:10.2f} ({ps:8.2f})  {tm:10.2f} ({tsp:8.2f})  {pm / tm:10.2f}  {'yes' if ok else 'NO'}")
    lines.append("# slower than the parent beyond its spread: " + (", ".join(f"{a} n={b} k={c}" for a, b, c in slower) if slower else "nowhere"))
    lines.append("# this build, one more call per shape: milliseconds per kernel (HIP events on the stream, all launches of the call)")
    lines += [kernels[k][len("KERNELS "):] for k in sorted(kernels, key=lambda c: (c[0], int(c[1]), int(c[2])))]
    lines.append("# the same with option cluster_walk = 1 (every cluster walks its members from position 0; one round): call_ms, then the kernels")
    lines += [f"{k[0]} {k[1]} {k[2]} call={plain[k + ('call',)]} " + " ".join(plain[k].split()[4:]) for k in sorted((c for c in plain if len(c) == 3), key=lambda c: (c[0], int(c[1]), int(c[2])))]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "cluster_timing.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        driver()
