"""GPU-box helper: searches by row id (freddy_gpu_ivfadc_search_ids / _pv_ids) on the bench workload (3 M x 300, C = 1000, m = 12,
K = 1024, W = 10, k = 5) with the whole table pinned as the vector handle, at Q in {1, 64, 1024, 4096, 8192} queries per call:
  (a) search(x)          the host-buffer call with pageable host vectors
  (b) search(xh[rows])   the same plus the host's gather of the rows out of its 3.6 GB copy -- what a caller that starts from ids pays
  (c) search_ids(ids)    4 bytes per query up, the rows gathered on the device
  (c') search_ids(ids)   after 3000 rows spread over the table were removed from the vector handle: its ids have gaps, a row is no longer
                         id - 1 (the lookup: csrc/internal.h row_of_near)
and the same for search_pv / search_pv_ids at pvf = 20; the bytes that cross PCIe per call (counted from the shapes), and the gather
kernel's own time (the handle's profile: device events) with the bytes it moves set against the HBM peak.

A process binds one library, so every measurement runs in a child process of its own:
  query_ids_timing.py [--ab <library of the parent commit>] [--rounds R]
starts the children alternately (parent build, this build, parent build, ...; the parent's library runs (a) only) and writes
profiles/query_ids_timing.txt: per Q the medians of every round, the spread between the parent build's rounds (the margin a
difference has to exceed), (c) against the parent's (a), and this build's (a) against the parent's (a) -- the no-regression rows for
the code the query source was threaded through.  R defaults to 4: the spread is read off four rounds of the parent build.  N / REPS_S (seconds of calls per figure) from the environment for a smaller run."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (1, 64, 1024, 4096, 8192)
N, REPS_S = int(os.environ.get("N", 3000000)), float(os.environ.get("REPS_S", 0.4))
K, W, PVF, D, HBM_PEAK = 5, 10, 20, 300, 8.0e12
NEW = ["freddy_gpu_ivfadc_search_ids", "freddy_gpu_pq_search_ids", "freddy_gpu_ivfadc_search_pv_ids", "freddy_gpu_pq_search_pv_ids"]


def child():
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
    from freddy_amd import gpu, index_build as ib
    lib = gpu.load(optional=NEW)
    have_ids = hasattr(lib, NEW[0])
    note = lambda what: print(f"[{'this build' if have_ids else 'parent build'}] {what}", file=sys.stderr, flush=True)
    note("building the tables")
    dev = torch.device("cuda", 0)
    x = ib.make_corpus(N, seed=20260101, device=dev)
    # the tables are the same in every child: built once per box (the key: N and the source of the builder)
    cache = f"/tmp/freddy_query_ids_tab_{N}_{hashlib.sha1(open(ib.__file__, 'rb').read()).hexdigest()[:12]}.npz"
    if os.path.exists(cache):
        tab = dict(np.load(cache))
    else:
        tab = ib.build_ivf_index(x, C=1000, m=12, K=1024, train_size=min(N, 100000), iters=10, seed=2)
        tab = {n: np.asarray(v) for n, v in tab.items() if n in ("coarse", "codebook", "list_off", "ids", "codes")}
        np.savez(cache, **tab)
    xh = x.cpu().numpy()
    del x
    torch.cuda.empty_cache()
    ids = np.arange(1, N + 1, dtype=np.int32)
    rng = np.random.default_rng(7)
    qid = np.sort(rng.choice(ids, size=max(QS), replace=False)).astype(np.int32)
    hq = np.ascontiguousarray(xh[qid - 1])
    ivf = gpu.IVFIndex(tab["coarse"], tab["codebook"], tab["list_off"], tab["ids"], tab["codes"])
    vec = gpu.VectorIndex(ids, xh)

    def timed(call):
        call(); call()
        t = time.perf_counter(); call(); one = time.perf_counter() - t
        n = int(min(400, max(5, REPS_S / max(one, 1e-6))))
        ts = []
        for _ in range(n):
            t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)   # (every call is synchronous: it ends in a device synchronise)
        return statistics.median(ts) * 1e3

    res = {"have_ids": have_ids, "rows": {}}
    for Q in QS:
        note(f"Q = {Q}")
        r = {}
        q, qi = hq[:Q], qid[:Q]
        r["a"] = timed(lambda: ivf.search(q, K, W))
        r["a_pv"] = timed(lambda: ivf.search_pv(vec, q, K, PVF, W))
        if have_ids:
            r["b"] = timed(lambda: ivf.search(xh[qi - 1], K, W))
            r["c"] = timed(lambda: ivf.search_ids(vec, qi, K, W, rule=gpu.QIDS_POSITIONAL))
            r["c_pv"] = timed(lambda: ivf.search_pv_ids(vec, qi, K, PVF, W, rule=gpu.QIDS_POSITIONAL))
            gi, gd = ivf.search(q, K, W)
            _, ci, cd = ivf.search_ids(vec, qi, K, W, rule=gpu.QIDS_POSITIONAL)
            r["same_lists"] = bool(np.array_equal(gi, ci) and np.array_equal(gd.view(np.uint32), cd.view(np.uint32)))
            pi, ps = ivf.search_pv(vec, q, K, PVF, W)
            _, ci, cs = ivf.search_pv_ids(vec, qi, K, PVF, W, rule=gpu.QIDS_POSITIONAL)
            r["same_lists_pv"] = bool(np.array_equal(pi, ci) and np.array_equal(ps.view(np.uint32), cs.view(np.uint32)))
            ivf.profile_enable(True)
            for _ in range(5):
                ivf.search_ids(vec, qi, K, W, rule=gpu.QIDS_POSITIONAL)
            prof = ivf.profile_read()
            ivf.profile_enable(False)
            launches, ms = prof.get("query_gather", (0, 0.0))
            r["gather_launches_per_call"] = launches / 5
            r["gather_us_per_call"] = ms * 1e3 / 5
        res["rows"][str(Q)] = r
    if have_ids:   # last: a vector table whose ids have gaps (none of the query ids is removed)
        gone = np.setdiff1d(ids[::N // 3000], qid).astype(np.int32)
        vec.remove_rows(gone)
        for Q in QS:
            qi = qid[:Q]
            res["rows"][str(Q)]["c_gaps"] = timed(lambda: ivf.search_ids(vec, qi, K, W, rule=gpu.QIDS_POSITIONAL))
            _, ci, cd = ivf.search_ids(vec, qi, K, W, rule=gpu.QIDS_POSITIONAL)
            gi, gd = ivf.search(hq[:Q], K, W)
            res["rows"][str(Q)]["same_lists"] &= bool(np.array_equal(gi, ci) and np.array_equal(gd.view(np.uint32), cd.view(np.uint32)))
    print("RESULT " + json.dumps(res), flush=True)


def run_child(so):
    env = dict(os.environ)
    env.pop("FREDDY_GPU_SO", None)
    if so:
        env["FREDDY_GPU_SO"] = os.path.abspath(so)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"child ({so or 'this build'}) ended with status {p.returncode}: nothing more is started")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main(argv):
    base = argv[argv.index("--ab") + 1] if "--ab" in argv else None
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 4
    new, old = [], []
    for _ in range(rounds):
        if base:
            old.append(run_child(base))
        new.append(run_child(None))
    out = open(os.path.join(ROOT, "profiles", "query_ids_timing.txt"), "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")

    def col(runs, Q, key):
        return [r["rows"][str(Q)][key] for r in runs]

    fmt = lambda v: "/".join(f"{t:.4f}" for t in v)
    say(f"# searches by row id, {N} x {D}, C=1000 m=12 K=1024 W={W} k={K}; ms per call, the median of each round's calls ({rounds} rounds, every round a fresh process"
        + (", alternating with a build of the parent commit)" if base else ")"))
    say("# (a) search(host vectors)   (b) search(xh[rows]): the host's gather + (a)   (c) search_ids(ids)   (c') search_ids(ids), 3000 rows removed from the vector table")
    w = 7 * rounds + 1
    say(f"#     Q   {'(a) ms':{w}s} {'(b) ms':{w}s} {'(c) ms':{w}s} {'(c~) ms'.replace('~', chr(39)):{w}s} (c) q/s     (c)/(a)  (c)/(b)  (c')/(a)  same lists")
    for Q in QS:
        a, b, c, g = col(new, Q, "a"), col(new, Q, "b"), col(new, Q, "c"), col(new, Q, "c_gaps")
        ma, mb, mc, mg = (statistics.median(v) for v in (a, b, c, g))
        say(f"{Q:7d}   {fmt(a):{w}s} {fmt(b):{w}s} {fmt(c):{w}s} {fmt(g):{w}s} {Q / mc * 1e3:10.0f}  {mc / ma:7.3f}  {mc / mb:7.3f}  {mg / ma:8.3f}  {all(col(new, Q, 'same_lists'))}")
    say()
    say(f"# post verification at pvf = {PVF}: search_pv(host vectors) against search_pv_ids(ids)")
    say("#     Q   search_pv ms          search_pv_ids ms      ids q/s     ids/host  same lists")
    for Q in QS:
        a, c = col(new, Q, "a_pv"), col(new, Q, "c_pv")
        ma, mc = statistics.median(a), statistics.median(c)
        say(f"{Q:7d}   {fmt(a):{w}s}  {fmt(c):{w}s}  {Q / mc * 1e3:10.0f}  {mc / ma:8.3f}  {all(col(new, Q, 'same_lists_pv'))}")
    say()
    say("# bytes over PCIe per call, counted from the shapes (up: queries or row numbers, and for pv the lists the re-rank reads from the pinned block")
    say("# and the raw queries of stage two; down: lists, straggler words, for pv stage one's lists and the result rows with their counts)")
    say("#     Q   search up      search_ids up  either down   search_pv up   search_pv_ids up  either down")
    kc = K * PVF
    for Q in QS:
        down, down_pv = Q * K * 8 + (Q + 2) * 4, Q * kc * 8 + (Q + 2) * 4 + Q * (K * 8 + 8)
        say(f"{Q:7d}   {Q * D * 4:12d}   {Q * 4:12d}   {down:11d}   {2 * Q * D * 4 + Q * kc * 4:12d}   {2 * Q * 4 + Q * kc * 4:15d}   {down_pv:11d}")
    say()
    say("# the gather kernel (query_gather; the handle's profile: device events around the launch, five calls): per search_ids call")
    say("#     Q   launches   us        bytes moved (rows read + block written + row numbers)   GB/s      of the HBM peak (8 TB/s)")
    for Q in QS:
        l, us = statistics.median(col(new, Q, "gather_launches_per_call")), statistics.median(col(new, Q, "gather_us_per_call"))
        moved = 2 * Q * D * 4 + Q * 4
        say(f"{Q:7d}   {l:8.1f}   {us:8.2f}  {moved:12d}" + (f"{'':44s}{moved / (us * 1e-6) / 1e9:8.1f}  {moved / (us * 1e-6) / HBM_PEAK:8.4f}" if us > 0 else "   (one query is read where its row lies: no launch)"))
    if base:
        say()
        say("# against the parent commit's build, alternating on this box.  spread: (max - min) / median of the parent build's own rounds -- a difference")
        say("# inside it is no difference.  The rows of this build's (a) are the no-regression condition for the existing entry point.")
        say("#     Q   parent (a) ms         spread   this build (a) ms     (a) new/parent   (c) ms                (c)/parent (a)   parent search_pv ms   this build search_pv ms   new/parent")
        for Q in QS:
            pa, na, c = col(old, Q, "a"), col(new, Q, "a"), col(new, Q, "c")
            ppv, npv = col(old, Q, "a_pv"), col(new, Q, "a_pv")
            mpa = statistics.median(pa)
            say(f"{Q:7d}   {fmt(pa):{w}s}  {(max(pa) - min(pa)) / mpa:6.3f}   {fmt(na):{w}s}  {statistics.median(na) / mpa:14.3f}   {fmt(c):{w}s}  {statistics.median(c) / mpa:14.3f}   "
                f"{fmt(ppv):{w}s}  {fmt(npv):{w}s}  {statistics.median(npv) / statistics.median(ppv):9.3f}")
    out.close()


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        main(sys.argv[1:])
