"""GPU-box helper: text vectors from token ids (freddy_gpu_tokenize, freddy_gpu_ivfadc_search_texts) on the bench tables (3 M x 300,
C = 1000, m = 12, K = 1024, W = 10, k = 5) with the whole table pinned as the vector handle, for n_texts in {1, 1024, 100000} texts
of {1, 5, 50, 1000} tokens each (distinct ids, rows spread over the table), FREDDY_QIDS_TABLE_ORDER, normalised.  Variants, alternated
in ONE process, their results compared bit for bit before anything is timed:
  (a) tokenize(texts)                 ids up, vectors down
  (b) the host path it replaces       the rows gathered out of the host's 3.6 GB copy and the model's arithmetic (numpy, float32
                                      operations in the reference's order, vectorised ACROSS texts, one core); left out beyond
                                      5 M tokens per call, where one run takes minutes
  (c) search_texts(texts)             against (d) tokenize(texts) followed by search(vectors)
then per-kernel times from the vector handle's profile (device events around the launches), with tok_unit in both forms: a chain
of squares per lane over 64 texts (option tokenize_unit = 2) and a wave per text with lane 0 walking the chain (= 1).
Writes profiles/tokenize_timing.txt.  N / REPS_S (seconds of calls per figure) from the environment for a smaller run."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, REPS_S = int(os.environ.get("N", 3000000)), float(os.environ.get("REPS_S", 0.3))
N_TEXTS, TOKENS = (1, 1024, 100000), (1, 5, 50, 1000)
K, W, D, HOST_MAX_TOKENS = 5, 10, 300, 5000000


def main():
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
    from freddy_amd import gpu, index_build as ib
    gpu.load()
    note = lambda what: print(f"[tokenize_timing] {what}", file=sys.stderr, flush=True)
    note("building the tables")
    x = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0))
    tab = ib.build_ivf_index(x, C=1000, m=12, K=1024, train_size=min(N, 100000), iters=10, seed=2)
    tab = {n: np.asarray(v) for n, v in tab.items() if n in ("coarse", "codebook", "list_off", "ids", "codes")}
    xh = x.cpu().numpy()
    del x
    torch.cuda.empty_cache()
    ids = np.arange(1, N + 1, dtype=np.int32)
    ivf = gpu.IVFIndex(tab["coarse"], tab["codebook"], tab["list_off"], tab["ids"], tab["codes"])
    vec = gpu.VectorIndex(ids, xh)
    rng = np.random.default_rng(7)

    def texts_of(n, L):
        """n texts of L distinct ids each, a stride of 2971 rows apart from a random start: (ids, offsets)"""
        start = rng.integers(0, N, size=n, dtype=np.int64)
        rows = (start[:, None] + 2971 * np.arange(L, dtype=np.int64)[None, :]) % N
        return (rows + 1).astype(np.int32).reshape(-1), np.arange(n + 1, dtype=np.int64) * L

    def host_path(tok, n, L):
        """the gather and the model's arithmetic, vectorised across the texts of a chunk"""
        out = np.empty((n, D), np.float32)
        fn = np.float32(L)
        rows = np.sort(tok.reshape(n, L).astype(np.int64) - 1, axis=1)   # (ids 1 .. N: the row is id - 1; the distinct rows ascending)
        for t0 in range(0, n, 4096):
            r = rows[t0:t0 + 4096]
            acc = np.zeros((r.shape[0], D), np.float32)
            for j in range(L):
                acc = acc + xh[r[:, j]] / fn
            sq = np.zeros(r.shape[0], np.float32)
            for j in range(D):
                sq = sq + acc[:, j] * acc[:, j]
            ln = np.sqrt(sq.astype(np.float64)).astype(np.float32)
            out[t0:t0 + 4096] = acc / ln[:, None]
        return out

    def timed(call, budget=REPS_S):
        call()
        t = time.perf_counter(); call(); one = time.perf_counter() - t
        if one >= 1.0:   # (seconds per call: one figure)
            return one * 1e3
        n = int(min(200, max(3, budget / max(one, 1e-6))))
        ts = []
        for _ in range(n):
            t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)   # (every call is synchronous)
        return statistics.median(ts) * 1e3

    def kernels(texts, unit):
        vec.set_option("tokenize_unit", unit)
        vec.profile_enable(True)
        for _ in range(3):
            vec.tokenize(texts)
        prof = vec.profile_read()
        vec.profile_enable(False)
        vec.set_option("tokenize_unit", 0)
        return {name: ms * 1e3 / 3 for name, (launches, ms) in prof.items()}

    rows = []
    for n in N_TEXTS:
        for L in TOKENS:
            note(f"n_texts = {n}, tokens = {L}")
            tok, off = texts_of(n, L)
            texts = (tok, off)
            r = {"n": n, "L": L}
            gv, gc = vec.tokenize(texts)
            assert (gc == L).all()
            for unit in (1, 2):
                vec.set_option("tokenize_unit", unit)
                wv, _ = vec.tokenize(texts)
                vec.set_option("tokenize_unit", 0)
                assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), "the two forms of tok_unit differ"
            host = n * L <= HOST_MAX_TOKENS
            if host:
                hv = host_path(tok, n, L)
                assert np.array_equal(gv.view(np.uint32), hv.view(np.uint32)), "tokenize differs from the host path"
            ci, cd = ivf.search(gv, K, W)
            sc, si, sd = ivf.search_texts(vec, texts, K, W)
            assert np.array_equal(sc, gc) and np.array_equal(si, ci) and np.array_equal(sd.view(np.uint32), cd.view(np.uint32)), \
                "search_texts differs from tokenize + search"
            r["a"] = timed(lambda: vec.tokenize(texts))
            r["b"] = timed(lambda: host_path(tok, n, L), budget=0.0) if host else None
            r["c"] = timed(lambda: ivf.search_texts(vec, texts, K, W))
            r["d"] = timed(lambda: ivf.search(vec.tokenize(texts)[0], K, W))
            r["k0"], r["k1"] = kernels(texts, 2), kernels(texts, 1)
            rows.append(r)

    out = open(os.path.join(ROOT, "profiles", "tokenize_timing.txt"), "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")

    say(f"# text vectors from token ids, {N} x {D}; TABLE_ORDER, normalised; ms per call, the median of the calls of one process; every variant's")
    say("# result was compared bit for bit with tokenize's before it was timed")
    say("# (a) tokenize(texts)   (b) host: gather + the model's arithmetic in numpy, one core   (c) search_texts   (d) tokenize + search(vectors)")
    say(f"# the searches: IVFADC, C=1000 m=12 K=1024 W={W} k={K}")
    say("# n_texts  tokens      (a) ms       (b) ms    (a)/(b)    texts/s (a)       (c) ms       (d) ms    (c)/(d)")
    for r in rows:
        b = f"{r['b']:12.3f} {r['a'] / r['b']:10.3f}" if r["b"] is not None else f"{'-':>12s} {'-':>10s}"
        say(f"{r['n']:9d} {r['L']:7d} {r['a']:12.3f} {b} {r['n'] / r['a'] * 1e3:14.0f} {r['c']:12.3f} {r['d']:12.3f} {r['c'] / r['d']:10.3f}")
    say()
    say("# per kernel, us per tokenize call (the handle's profile: device events around each launch, three calls); tok_unit in both forms:")
    say("# lanes = a chain of squares per lane over 64 texts (tokenize_unit = 2), wave = a wave per text, lane 0 walks the chain (= 1);")
    say("# the default (0) takes the wave form below 16384 texts and the lane form from there on: (a), (c) and (d) above ran with it")
    say("# n_texts  tokens  tok_resolve     tok_rows  tok_centroid  tok_unit lanes  tok_unit wave   gathered GB/s (tok_centroid)")
    for r in rows:
        k0, k1 = r["k0"], r["k1"]
        moved = r["n"] * r["L"] * D * 4
        say(f"{r['n']:9d} {r['L']:7d} {k0.get('tok_resolve', 0):12.1f} {k0.get('tok_rows', 0):12.1f} {k0.get('tok_centroid', 0):13.1f} "
            f"{k0.get('tok_unit', 0):15.1f} {k1.get('tok_unit', 0):14.1f} {moved / max(k0.get('tok_centroid', 0), 1e-3) / 1e3:14.1f}")
    out.close()


if __name__ == "__main__":
    main()
