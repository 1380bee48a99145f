"""GPU-box helper: the batched approximate analogies on the bench table (3 M x 300, C = 1000, m = 12, K = 1024, W = 10), triples drawn
from indexed rows.  For pvf in {1, 6, 20, 100} (n_cand = pvf + 3, k = 1, what the reference's analogy_3cosadd_ivfadc passes) and
1 / 32 / 1024 triples per call: the time of one analogy_3cosadd_ivfadc_batch call (ONE freddy_gpu_ivfadc_analogy), of the same
triples through the loop of single analogy_3cosadd_ivfadc calls (one synchronous search and one host loop per triple: all the
library offered before) and through freddy_gpu_exact_analogy (3CosAdd over the whole table); the share of triples whose answer equals
the exact one; the share of the kernel time in aa_query / aa_rerank.  The three are timed alternately, REPS times each, medians.
Writes profiles/approx_analogy_timing.txt.  N / REPS from the environment for a smaller run."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
from freddy_amd import gpu, index_build as ib, udf   # noqa: E402

N, REPS = int(os.environ.get("N", 3000000)), int(os.environ.get("REPS", 3))
W = 10
dev = torch.device("cuda", 0)
out = open(os.path.join(ROOT, "profiles", "approx_analogy_timing.txt"), "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(f):
    t = time.perf_counter()
    r = f()
    return time.perf_counter() - t, r


t0 = time.time()
x = ib.make_corpus(N, seed=20260101, device=dev)
tab = ib.build_ivf_index(x, C=1000, m=12, K=1024, train_size=100000, iters=10, seed=2)
xh = x.cpu().numpy()
del x
ids = np.arange(1, N + 1, dtype=np.int32)
triples = np.random.default_rng(7).choice(ids, (1024, 3)).astype(np.int32)
vec = gpu.VectorIndex(ids, xh)
s = udf.Session()
s.load_vecs_norm(ids, xh)
s.load_ivfadc(tab["coarse"], tab["codebook"], tab["ids"], np.repeat(np.arange(1000), np.diff(tab["list_off"])).astype(np.int32), tab["codes"])
s.set_w(W)
s.analogy_3cosadd_ivfadc_batch(triples[:1])           # pins google_vecs_norm behind the session
ivf = s.gpu_index("ivfadc")
say(f"# approximate analogies (3CosAdd over IVFADC candidates), {N} x 300, C=1000 m=12 K=1024 W={W} k=1 n_cand=pvf+3, medians of {REPS} alternating repetitions (setup {time.time() - t0:.0f} s)")
say("# pvf  triples  batch_call_ms  batch_k_per_s  single_loop_ms  loop/batch  exact_3cosadd_ms  exact/batch  equals_exact  aa_query_ms  aa_rerank_ms  aa_share_of_kernels")
exact_ids = vec.analogy(triples, 1, "3cosadd")[0][:, 0]
for pvf in (1, 6, 20, 100):
    s.set_pvf(pvf)
    for Q in (1, 32, 1024):
        t = triples[:Q]
        got = s.analogy_3cosadd_ivfadc_batch(t)        # warm-up
        s.analogy_3cosadd_ivfadc(*t[0].tolist())
        vec.analogy(t, 1, "3cosadd")
        t_b, t_l, t_e = [], [], []
        for _ in range(REPS):
            t_b.append(timed(lambda: s.analogy_3cosadd_ivfadc_batch(t))[0])
            dt, loop = timed(lambda: [s.analogy_3cosadd_ivfadc(*tr) for tr in t.tolist()])
            t_l.append(dt)
            t_e.append(timed(lambda: vec.analogy(t, 1, "3cosadd"))[0])
        assert got.tolist() == loop, "the batch and the loop of single calls disagree"
        ivf.profile_enable(True)
        s.analogy_3cosadd_ivfadc_batch(t)
        prof = ivf.profile_read()
        ivf.profile_enable(False)
        all_ms = sum(ms for _, ms in prof.values())
        q_ms, r_ms = prof["aa_query"][1], prof["aa_rerank"][1]
        b, l, e = (statistics.median(v) * 1e3 for v in (t_b, t_l, t_e))
        say(f"{pvf:5d}  {Q:7d}  {b:13.3f}  {Q / b:13.1f}  {l:14.2f}  {l / b:10.1f}  {e:16.2f}  {e / b:11.1f}  {float((got == exact_ids[:Q]).mean()):12.4f}  "
            f"{q_ms:11.4f}  {r_ms:12.4f}  {(q_ms + r_ms) / all_ms if all_ms else 0:19.3f}")
        if Q == 1024:
            say("#        kernels: " + ", ".join(f"{n} {ms:.3f} ms" for n, (_, ms) in sorted(prof.items())))
            say(f"#        stats: {ivf.last_approx_analogy_stats()}")
out.close()
